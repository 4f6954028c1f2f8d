"""Every selectable instantiation of the streamed kernel (bp_decode_kernel), the per-pass kernels (bp_spread_*), the on-chip serial_relative
kernel (bp_relative_lds_kernel), the other serial families and the slot kernel, for product-sum, product-sum with fast math and min-sum, and the
wavefront ladders once more with fast math -- each on a smallest code that selects it (tests/stream_ladder_util.py; tests/test_stream_ladder_cases.py
checks the cases themselves without a GPU).

Exact math: the decode equals the oracle's bit for bit -- decisions, iteration counts, converge flags, log-ratios as bit patterns, for serial_relative the
order the last row leaves -- and the launch log shows EXACTLY the named instantiations, as often as the host code launches them, and no other
instantiation of any decode family.  Every streamed case also equals the same decode on the per-pass kernels, every on-chip serial_relative case the
per-lane kernel (REL_LDS 0).
Fast math: decisions, iteration counts and converge flags equal the exact oracle's (the CPU test asserts that the oracle with the device's fast
routines plugged in agrees with it there), the log-ratios lie within llr_close(rtol = 1e-5) of the exact oracle's (LLR_RTOL), the
log names the <0, 1, ...> instantiation; the largest relative difference against the FAST oracle, and whether the bits are equal, are printed (NOTES.md
holds one box's figures) and not asserted.
The LOOP forms of the per-pass kernels: a second pass whose compacted list of tiles is longer than 32, so that the looping launches have tiles to do."""
import functools

import numpy as np
import pytest

import launch_util
import stream_ladder_util as su
from golden_util import llr_close

pytestmark = pytest.mark.gpu

_M = {"product_sum": 0, "minimum_sum": 1}
FAST_REPORT = {}  # family -> [largest relative difference against the fast oracle, cases, cases whose log-ratio bits equal the fast oracle's]


def _ids(cases):
    return [c.id for c in cases]


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _decode(case, **override):
    """One decode of the case's inputs on a new handle, set up as the case says (override: fields of the case replaced) -> (outputs, final order or None, log)."""
    from ldpc_amd.engine import HipBpEngine
    c = case._replace(**override)
    h, probs, synd, row_probs = su.inputs(case.id)
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], probs, su.MAX_ITER, _M[c.method], c.alpha)
    try:
        if c.math:
            eng.set_math("fast")
        if c.schedule != "parallel":
            eng.set_schedule(c.schedule)
        for setter, value in ((eng.set_small_code_kernel, c.mode), (eng.set_handoff, c.handoff), (eng.set_ring, c.ring), (eng.set_serial_kernel, c.serial_kernel),
                              (eng.set_repack, c.repack)):
            if value is not None:
                setter(value)
        for name, value in c.switches.items():
            eng.set_debug_switch(name, value)
        with launch_util.launch_log() as log:
            out = eng.decode_batch(synd) if row_probs is None else eng.decode_batch(synd, channel_probs=row_probs)
        order = eng.schedule_order() if c.schedule == "serial_relative" else None
    finally:
        eng.close()
    return tuple(np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in out), order, log


def _same(got, want, who, method):
    """As tests/test_gpu_instantiations.py: _same."""
    for k, name in ((0, "decoding"), (2, "iterations"), (3, "converge")):
        assert np.array_equal(got[k], np.asarray(want[k]).astype(got[k].dtype)), f"{name}: {who}"
    differ = _bits(got[1]) != _bits(want[1])
    if method == "product_sum":  # (any NaN matches any NaN: the payload of inf - inf depends on the operand order -- oracle.bits_equal)
        differ &= ~(np.isnan(got[1]) & np.isnan(want[1]))
    assert not differ.any(), f"log-ratios (bit patterns): {who}: {int(differ.sum())} of {differ.size} differ, first at {tuple(np.argwhere(differ)[0])}"


def _fast_report(key, family, got_llr, fast_llr):
    """Print (never assert) how far the kernel's fast math is from the fast oracle's."""
    both = np.isfinite(got_llr) & np.isfinite(fast_llr) & (fast_llr != 0)
    rel = float(np.max(np.abs(got_llr[both] - fast_llr[both]) / np.abs(fast_llr[both]))) if both.any() else 0.0
    equal = bool(np.all((_bits(got_llr) == _bits(fast_llr)) | (np.isnan(got_llr) & np.isnan(fast_llr))))
    print(f"[fast math] {key}: largest relative difference against the fast oracle {rel:.3e}; bits equal: {equal}")
    rec = FAST_REPORT.setdefault(family, [0.0, 0, 0])
    rec[0], rec[1], rec[2] = max(rec[0], rel), rec[1] + 1, rec[2] + int(equal)


def _same_fast(got, exact, who):
    for k, name in ((0, "decoding"), (2, "iterations"), (3, "converge")):
        assert np.array_equal(got[k], np.asarray(exact[k]).astype(got[k].dtype)), f"{name}: {who}"
    assert llr_close(got[1], exact[1], rtol=1e-5), f"log-ratios beyond 1e-5 relative of the exact oracle's: {who}"


def _assert_log(case, log):
    launch_util.assert_resolved(log)
    ran = launch_util.of(log, *su.FAMILY_KERNELS)
    assert ran == sorted(case.launches), f"expected exactly {sorted(case.launches)}; the log has {ran}"
    for name, count in case.launches.items():
        assert count is None or log[name] == count, f"{name}: {log[name]} launches, expected {count}"
    if case.id in su.NOT_SELECTABLE:
        name, why = su.NOT_SELECTABLE[case.id]
        assert name not in log, f"{name} ran, but is listed as not selectable: {why}"


@functools.lru_cache(maxsize=None)
def _per_lane_relative(case_id):
    """The per-lane serial_relative kernel on a case's inputs (the cases of one shape and method share them: same seed, same builder)."""
    out, order, log = _decode(su.BY_ID[case_id], switches={"REL_LDS": 0})
    launch_util.assert_ran(log, "bp_serial_relative_kernel")
    launch_util.assert_not_ran(log, "bp_relative_lds_kernel")
    return out, order


def _check(case):
    got, order, log = _decode(case)
    want = su.expected(case.id)
    if case.math:
        _same_fast(got, want, "kernel (fast math) vs exact oracle")
        _fast_report(case.id, case.family, got[1], su.expected_fast(case.id)[1])
    else:
        _same(got, want, "kernel vs oracle", case.method)
    if case.schedule == "serial_relative":
        assert np.array_equal(order, want[4]), "the order the last row leaves"
    _assert_log(case, log)
    if case.cross == "per_pass":
        other, _, other_log = _decode(case, handoff=1000)
        _same(got, other, "streamed kernel vs per-pass kernels", case.method)
        launch_util.assert_not_ran(other_log, "bp_decode_kernel")
        launch_util.assert_ran(other_log, "bp_spread_check_kernel", "bp_spread_bit_kernel")
    elif case.cross == "rel0":
        first = next(c for c in su.REL_CASES if (c.method, c.math, c.seed) == (case.method, case.math, case.seed))
        other, other_order = _per_lane_relative(first.id)
        _same(got, other, "on-chip kernel vs per-lane kernel (REL_LDS 0)", case.method)
        assert np.array_equal(order, other_order), "final order: on-chip kernel vs per-lane kernel"


@pytest.mark.parametrize("case", su.DECODE_CASES, ids=_ids(su.DECODE_CASES))
def test_streamed_kernel_instantiation(case, oracle_built):
    _check(case)


@pytest.mark.parametrize("case", su.SPREAD_CASES, ids=_ids(su.SPREAD_CASES))
def test_per_pass_kernel_instantiations(case, oracle_built):
    _check(case)  # (bp_decode_kernel is absent: _assert_log allows no instantiation beyond the five per-pass names)


@pytest.mark.parametrize("case", su.REL_CASES, ids=_ids(su.REL_CASES))
def test_relative_lds_kernel_instantiation(case, oracle_built):
    _check(case)


@pytest.mark.parametrize("case", su.SERIAL_CASES, ids=_ids(su.SERIAL_CASES))
def test_serial_and_slot_kernel_instantiation(case, oracle_built):
    _check(case)


@pytest.mark.parametrize("case", su.FAST_WAVE_CASES, ids=_ids(su.FAST_WAVE_CASES))
def test_wave_kernel_rung_with_fast_math(case, oracle_built):
    _check(case)


@pytest.mark.parametrize("case", su.LOOP_CASES, ids=_ids(su.LOOP_CASES))
def test_looping_forms_of_a_compacted_second_pass(case, oracle_built):
    """An easy batch steers the next decode on the handle into a second pass with compacted late rounds; the hard batch then keeps more than 32 tiles
    alive 8 rounds into that pass, so the looping launches (slots 32 ..) carry tiles.  The steered decode equals the plain one bit for bit."""
    from ldpc_amd.engine import HipBpEngine
    h, easy, hard, hopeless = su.loop_inputs(case.id)
    n = h.shape[1]
    eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, su.LOOP_P), su.LOOP_MAX_ITER, _M[case.method], case.alpha)
    try:
        eng.set_small_code_kernel(0)
        if case.math:
            eng.set_math("fast")
        eng.set_debug_switch("SPREAD_NT", case.nt)
        eng.set_debug_switch("REPACK_MIN_TILES", 1)
        decode = lambda s: tuple(np.asarray(x) for x in eng.decode_batch(s))
        eng.set_repack(0)
        ref = decode(hard)
        # on the CPU, before the case is trusted: more than 32 x 64 rows run to the last iteration -- whatever the cut, they are alive 8 rounds into a second pass
        running = ~ref[3].astype(bool) & (ref[2] == su.LOOP_MAX_ITER)
        print(f"{case.id}: {int(running.sum())} of {len(hard)} rows run to iteration {su.LOOP_MAX_ITER}; {int(ref[3].sum())} converge")
        assert running.sum() > 32 * 64 and running[hopeless].all() and ref[3].any()
        want = su.loop_expected(case.id)
        sample = tuple(x[su.LOOP_SAMPLE] for x in ref)
        if case.math:
            _same_fast(sample, want, "plain decode vs exact oracle")
            _fast_report(case.id, "spread (LOOP)", sample[1], su.loop_expected(case.id, True)[1])
        else:
            _same(sample, want, "plain decode vs oracle", case.method)
        eng.set_repack(-1)
        first = decode(easy)  # no histogram yet: a plain decode, which leaves one
        late = int((~first[3].astype(bool)).sum() + (first[3].astype(bool) & (first[2] >= 11)).sum())
        assert 1 <= late <= 24 and (first[2][first[3].astype(bool)] == 1).all(), late  # (stream_first_pass_length: late_rows; stream_rounds: may_compact)
        with launch_util.launch_log() as log:
            got = decode(hard)
    finally:
        eng.close()
    _same(got, ref, "steered two-pass decode vs plain decode", case.method)
    launch_util.assert_ran(log, "gather_lane_state_kernel", "bp_spread_compact_kernel")
    ran = set(launch_util.of(log, "bp_spread_check_kernel", "bp_spread_bit_kernel", "bp_spread_synd_kernel", "bp_spread_finish_kernel"))
    assert ran == su.loop_launches(case), f"expected exactly {sorted(su.loop_launches(case))}; the log has {sorted(ran)}"


def test_zz_fast_math_report():
    """Printed last: per family, how far the kernels' fast math was from the fast oracle in the cases above (a figure, not an assertion)."""
    for family, (rel, cases, equal) in sorted(FAST_REPORT.items()):
        print(f"[fast math] family {family}: largest relative difference against the fast oracle {rel:.3e} over {cases} cases; bits equal in {equal}")
