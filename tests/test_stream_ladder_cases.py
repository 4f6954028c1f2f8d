"""The cases of tests/test_gpu_stream_instantiations.py checked WITHOUT a GPU, from the builders (tests/stream_ladder_util.py) and the oracle
alone: every matrix has the shape its case states, the oracle converges on some rows and not on others, every instantiation the library
holds of the walked templates is named by a case (or listed as not selectable), and every fast-math case meets the precondition that makes
its GPU assertion safe: the exact oracle and the oracle with the device's fast routines plugged in (oracle/bp_oracle.c: bp_oracle_set_math,
which the parallel loop and every serial schedule's product-sum site honour) agree in decisions, iteration counts, converge flags -- the final
order of serial_relative included -- and in their log-ratios within llr_close(rtol = 1e-5)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ladder_util as lu
import stream_ladder_util as su
from golden_util import llr_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ids(cases):
    return [c.id for c in cases]


FAST_CASES = [c for c in su.ALL_CASES if c.math == 1]


def _named():
    named = {k for c in su.ALL_CASES for k in c.launches}
    for c in su.LOOP_CASES:
        named |= su.loop_launches(c)
    return named


def test_case_tables_name_what_they_should():
    assert len(set(_ids(su.ALL_CASES))) == len(su.ALL_CASES) and len(set(_ids(su.LOOP_CASES))) == len(su.LOOP_CASES)
    named = _named()
    count = lambda base: len({k for k in named if k.split("<")[0] == base})
    # bp_decode_kernel: 3 pairs x (6 register rungs + the variable ring) + the rings: 5 product-sum, 5 product-sum fast, 3 min-sum = 34; two more are compiled
    # that no rule selects
    assert count("bp_decode_kernel") == 34 and all(k not in named for k, _ in su.NOT_SELECTABLE.values())
    assert set(su.NOT_SELECTABLE) <= set(su.BY_ID)
    # 3 pairs x: DR 8 / 16 x NT x LOOP;  DC 4 / 8 x NT x (plain, LOOP, RP);  RP;  and <LOOP, RP> / <LOOP> of finish and synd
    assert count("bp_spread_check_kernel") == 24 and count("bp_spread_bit_kernel") == 36 and count("bp_spread_init_kernel") == 6
    assert count("bp_spread_finish_kernel") == 3 and count("bp_spread_synd_kernel") == 2
    assert count("bp_relative_lds_kernel") == 48  # 3 pairs x (GS 64: DR 4 / 8 / 16 x DC 2 / 4 / 8; GS 16: DR 4 / 8 / 16; EXT: DR 8 / 16 x DC 4 / 8)
    assert count("bp_serial_kernel") == 9 and count("bp_serial_level_kernel") == 9 and count("bp_serial_stream_kernel") == 6
    assert count("bp_serial_stream_var_kernel") == 6 and count("bp_serial_lane_var_kernel") == 6 and count("bp_serial_lane_kernel") == 3
    assert count("bp_serial_relative_kernel") == 3 and count("serial_edge0_kernel") == 3 and count("serial_var_init_kernel") == 3
    assert count("bp_small_kernel") == 6 and count("bp_edge0_kernel") == 3
    # the wavefront ladders with fast math: every product-sum rung of tests/ladder_util.py once more
    assert count("bp_wave_kernel") == 10 and count("bp_wave_ps_kernel") == 12
    # every exact case of the streamed kernel is cross-checked on the per-pass kernels, every exact on-chip serial_relative case on the per-lane kernel
    assert all((c.cross == "per_pass") == (c.math == 0) for c in su.DECODE_CASES) and all((c.cross == "rel0") == (c.math == 0) for c in su.REL_CASES)


def test_every_instantiation_the_library_holds_is_named_or_listed_as_not_selectable():
    """The kernels the built library can launch (the kernel handles of its dynamic symbol table), against the case tables: nothing compiled
    is forgotten.  (An instantiation that no host rule refers to has device code but no handle: those are what tools/instantiation_coverage.py
    marks "not selectable" from the compiler's listing -- NOT_SELECTABLE here, each kept true by a GPU case.)"""
    lib = os.path.join(ROOT, "ldpc_amd", "lib", "libldpc_hip.so")
    assert os.path.exists(lib), "build() leaves the library there"
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "binutils' nm (or llvm-nm) is needed to list the library's kernel handles"
    out = subprocess.run([nm, "-D", "--defined-only", "-C", lib], capture_output=True, text=True, check=True).stdout
    held = set()
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ [VvBbDd] (?:void )?(\w+<[^(]*>)\(", line)
        if m:
            held.add(m.group(1))
    named = _named() | {k for c in lu.ALL_CASES for k in ([c.kernel] if c.kernel else [])}
    walked = su.WALKED_TEMPLATES + ("bp_wave_kernel", "bp_wave_ps_kernel")
    for base in walked:
        assert any(k.split("<")[0] == base for k in held), f"no handle of {base} in the library's symbol table"
    not_selectable = {k for k, _ in su.NOT_SELECTABLE.values()}
    forgotten = sorted(k for k in held if k.split("<")[0] in walked and k not in named and k not in not_selectable)
    assert not forgotten, f"compiled, but no case names them: {forgotten}"
    unknown = sorted(k for k in named if k.split("<")[0] in walked and k not in held)
    assert not unknown, f"named by a case, but not in the library: {unknown}"
    assert not (not_selectable & held), "an instantiation listed as not selectable has a host rule after all"


@pytest.mark.parametrize("case", su.ALL_CASES, ids=_ids(su.ALL_CASES))
def test_builder_gives_the_stated_shape(case):
    h, probs, synd, row_probs = su.inputs(case.id)
    rows, cols = np.asarray(h.sum(axis=1)).ravel(), np.asarray(h.sum(axis=0)).ravel()
    if case.regular:
        n, dv, dc, _ = case.regular
        assert h.shape == (n * dv // dc, n) and (rows == dc).all() and (cols == dv).all()
    else:
        b = case.build
        assert h.shape[0] == b["m"] and rows.max() == b["max_row"] and rows.min() == b["min_row"] and cols.max() == b["max_col"] and cols.min() == 1
    if case.math:  # fast math: no weight-1 column under a weight-2 check (no weight-2 check at all)
        assert rows.min() >= 3
    assert synd.shape == (su.BATCH, h.shape[0]) and not synd[0].any() and (synd[su.BAD_ROWS[0]] == 2).sum() == 1 and (synd[su.BAD_ROWS[1]] == 3).sum() == 1
    assert case.uniform == (len(set(probs.tolist())) == 1)
    if not case.uniform:
        assert (probs == 0.5).sum() == 1 and (probs == 0.7).sum() == 1
    assert (row_probs is not None) == bool(case.rp)
    if case.rp:
        assert row_probs.shape == (su.BATCH, h.shape[1]) and len({r.tobytes() for r in row_probs}) == su.BATCH
        assert (row_probs == 0.5).sum() == 1 and (row_probs == 0.7).sum() == 1


@pytest.mark.parametrize("case", su.ALL_CASES, ids=_ids(su.ALL_CASES))
def test_expected_names_follow_the_size_rules(case):
    """The names in the tables against the restated rules applied to the matrix the builder really gave."""
    h = su.matrix(case.id)
    dr, dc = int(h.sum(axis=1).max()), int(h.sum(axis=0).max())
    sw = case.switches
    if case.family == "decode":
        name, ring = su.decode_kernel(case.method, case.math, dr, dc, ring=case.ring or 0, regular=bool(case.regular), var_ring=bool(sw.get("VAR_RING")))
        assert name in case.launches and (f"bp_edge0_kernel<{su._M[case.method]}, {case.math}>" in case.launches) == (ring > 0)
        if case.id in su.NOT_SELECTABLE:
            assert su.NOT_SELECTABLE[case.id][0] not in case.launches
    elif case.family == "spread":
        assert case.launches == su.per_pass_launches(case.method, case.math, dr, dc, sw["SPREAD_NT"], bool(case.rp))
    elif case.family == "rel":
        gs, ext = sw.get("REL_LDS", 64), sw.get("REL_EXT", 0)
        assert su.rel_kernel(case.method, case.math, dr, dc, gs, ext) in case.launches
        assert ext or su.rel_lds_fits(h.shape[0], h.shape[1], h.nnz, dc, case.method == "product_sum", gs)
        assert h.shape[1] < 65535 and h.nnz < 65535 and dr <= 16 and dc <= 8
    elif case.family == "serial" and case.schedule == "serial":
        (name,) = [k for k in case.launches if k.startswith("bp_serial")]
        if case.serial_kernel in (0, 1):
            assert name.endswith(f", {su.serial_rung(dr, dc)}>")
        elif case.regular:
            assert (dr, dc) == (6, 3)
        else:  # plan_serial_stream: the item form
            assert name.endswith(f", {8 if dr <= 8 else 16}, {4 if dc <= 4 else 8}>") and dr <= 16 and dc <= 8


@pytest.mark.parametrize("case", su.ALL_CASES, ids=_ids(su.ALL_CASES))
def test_oracle_converges_on_some_rows_and_not_on_others(case, oracle_built):
    conv = np.asarray(su.expected(case.id)[3]).astype(bool)
    assert not conv[list(su.BAD_ROWS)].any()
    others = np.delete(conv, su.BAD_ROWS)
    assert others.any() and not others.all()


@pytest.mark.parametrize("case", FAST_CASES, ids=_ids(FAST_CASES))
def test_fast_math_precondition(case, oracle_built):
    """What makes the GPU assertion of a fast-math case safe: the exact oracle decides, counts and flags as the fast oracle does."""
    exact, fast = su.expected(case.id), su.expected_fast(case.id)
    assert np.array_equal(exact[0], fast[0]), "decisions"
    assert np.array_equal(exact[2], fast[2]), "iteration counts"
    assert np.array_equal(exact[3], fast[3]), "converge flags"
    assert llr_close(fast[1], exact[1], rtol=1e-5), "log-ratios beyond 1e-5 relative"
    if case.schedule == "serial_relative":
        assert np.array_equal(exact[4], fast[4]), "final order"


@pytest.mark.parametrize("case", su.LOOP_CASES, ids=_ids(su.LOOP_CASES))
def test_loop_case_inputs(case, oracle_built):
    """The easy batch leaves few enough stragglers for the late rounds to compact (stream_first_pass_length: at most 24 rows unconverged or
    converging 11 iterations in or later -- a cut lies at 2 or beyond), the hard batch more than 32 x 64 rows that never converge."""
    h, easy, hard, hopeless = su.loop_inputs(case.id)
    rows, cols = np.asarray(h.sum(axis=1)).ravel(), np.asarray(h.sum(axis=0)).ravel()
    assert rows.max() == case.build["max_row"] and cols.max() == case.build["max_col"] and h.shape[1] >= 140
    assert su.LOOP_BATCH // 64 + 1 > 40 and len(hopeless) > 32 * 64 and (hard[hopeless] == 2).sum(axis=1).all()
    o = oracle_built.BpOracle(h, error_rate=su.LOOP_P, max_iter=su.LOOP_MAX_ITER, bp_method=case.method, ms_scaling_factor=case.alpha)
    with np.errstate(all="ignore"):
        _, _, it, cv = o.decode_batch(easy)
    late = int((~cv).sum() + (cv & (it >= 11)).sum())
    assert su.LOOP_EASY_HOPELESS <= late <= 24, late
    assert (it[cv] <= 4).mean() > 0.9  # ... and most of the rest converges at once: a cut pays
    exact = su.loop_expected(case.id)
    assert exact[3].any() and not exact[3].all()  # the sample of the hard batch holds rows that converge and rows that do not
    if case.math:  # the fast-math precondition, on the sample the GPU test compares
        fast = su.loop_expected(case.id, True)
        assert all(np.array_equal(exact[k], fast[k]) for k in (0, 2, 3)) and llr_close(fast[1], exact[1], rtol=1e-5)
