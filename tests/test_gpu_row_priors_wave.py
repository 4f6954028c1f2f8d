"""``decode_batch(..., channel_probs=P)`` with min-sum on the codes of the lane = node kernel: bp_wave_rp_kernel<DR, DC, TEAM>
(ldpc_amd/csrc/bp_wave_rp_kernel.h) against the per-row oracle and the reference's own fixtures -- hard decisions, converge flags, iteration
counts and the bit patterns of the log-ratios, every row -- on the cases of tests/row_priors_wave_util.py (tests/test_row_priors_wave_cases.py
checks them without a GPU), with the launch log showing that exactly the named instantiation ran.  Then what is new about the route: the
code whose slot does not fit the slot kernel; a wavefront or team must read the priors of the row it PULLED (static teams, work pools,
20 011 rows); ``row_prior_route`` against the launch log in every mode; a handle that goes from plain to row-prior decodes and back; the
query through every layer."""
import numpy as np
import pytest
import scipy.sparse as sp

import ladder_util as lu
import launch_util
import row_priors_edge_util as eu
import row_priors_wave_util as ru
from oracle import bits_equal
from row_priors_util import llr_digest, ran_bp

pytestmark = pytest.mark.gpu

ONCHIP_PLAIN = ("bp_edge_kernel", "bp_edge8_kernel", "bp_wave_kernel", "bp_wave_ps_kernel")  # kernels that read the handle's priors only
PER_PASS = ("bp_spread_init_kernel", "bp_spread_check_kernel", "bp_spread_bit_kernel", "bp_spread_finish_kernel", "bp_spread_synd_kernel", "bp_decode_kernel")
ROUTES = ("per_pass", "bp_edge", "bp_edge8", "bp_wave", "bp_wave_team", "bp_small")
MODES = (-1, 0, 1, 2, 3, 4, 5, 6)


def _engine(h, own, max_iter, alpha, method="minimum_sum", mode=None, switches=None):
    from ldpc_amd.engine import HipBpEngine
    h = sp.csr_matrix(h)
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], np.asarray(own, np.float64), max_iter, 0 if method == "product_sum" else 1, alpha)
    if mode is not None:
        eng.set_small_code_kernel(mode)
    for name, value in (switches or {}).items():
        eng.set_debug_switch(name, value)
    return eng


def _np(x):
    return None if x is None else x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same(got, want, what, want_llr=True):
    dec, llr, it, cv = (_np(x) for x in got)
    if not want_llr:
        assert llr is None
        llr = want[1]
    print(f"{what}: {int((dec != want[0]).any(axis=1).sum())} rows differ in decisions, {int(np.count_nonzero(cv.astype(bool) != want[3]))} in flags, "
          f"{int(np.count_nonzero(it != want[2]))} in iteration counts, {int(np.count_nonzero(llr_digest(llr) != llr_digest(want[1])))} in log-ratio bits, of {len(dec)}")
    assert np.array_equal(dec, want[0]), f"{what}: hard decisions"
    assert np.array_equal(cv.astype(bool), want[3]), f"{what}: converge flags"
    assert np.array_equal(it, want[2]), f"{what}: iteration counts"
    assert bits_equal(llr, want[1]), f"{what}: log-ratios differ in some bit"


def _assert_rp(log, name):
    """Exactly the named instantiation of bp_wave_rp_kernel, once, behind its prior table; no other BP decode kernel."""
    launch_util.assert_resolved(log)
    assert launch_util.of(log, ru.RP_KERNEL) == [name], f"expected exactly {name}; the log has {sorted(log)}"
    assert log[name] == 1
    launch_util.assert_not_ran(log, *lu.BP_DECODE_KERNELS, *eu.RP_KERNELS, "row_priors_kernel", "row_priors_rowmajor_kernel", "wave_prior_pad_kernel")
    launch_util.assert_ran(log, "wave_rp_prior_kernel")


def _route_of(log):
    """The route a launch log shows."""
    launch_util.assert_resolved(log)
    launch_util.assert_not_ran(log, *ONCHIP_PLAIN)
    wave, small = launch_util.of(log, ru.RP_KERNEL), launch_util.of(log, "bp_small_kernel")
    edge, edge8, per_pass = launch_util.of(log, "bp_edge_rp_kernel"), launch_util.of(log, "bp_edge8_rp_kernel"), launch_util.of(log, *PER_PASS)
    families = [bool(wave), bool(small), bool(edge), bool(edge8), bool(per_pass)]
    assert sum(families) == 1, f"one kernel family per decode; the log has {sorted(log)}"
    if wave:
        assert len(wave) == 1
        return "bp_wave_team" if wave[0].endswith(", true>") else "bp_wave"
    if small:
        assert all(k.endswith(", true>") for k in small), small
        return "bp_small"
    return "bp_edge" if edge else "bp_edge8" if edge8 else "per_pass"


def _decode(name, mode, switches=None, alpha=ru.ALPHA, method="minimum_sum", rows=None, **kw):
    c = ru.case(name)
    rows = slice(None) if rows is None else rows
    eng = _engine(c["h"], c["own"], ru.MAX_ITER, alpha, method, mode, switches)
    try:
        with launch_util.launch_log() as log:
            out = eng.decode_batch(np.ascontiguousarray(c["synd"][rows]), channel_probs=np.ascontiguousarray(c["probs"][rows]), **kw)
    finally:
        eng.close()
    return out, log


# ---- 1. every instantiation --------------------------------------------------------------------------------------------------------------
_SEEN = set()


@pytest.mark.parametrize("mode", [4, 5], ids=["mode4-wavefront", "mode5-team"])
@pytest.mark.parametrize("name", list(ru.CASES))
def test_every_instantiation(name, mode):
    kernel = ru.kernel_name(ru.CASES[name][0], mode == 5)
    for want_llr in (True, False):
        got, log = _decode(name, mode, want_llr=want_llr)
        _same(got, ru.expected(name), f"{name}, mode {mode}, {'with' if want_llr else 'without'} log-ratios", want_llr)
        _assert_rp(log, kernel)
    _SEEN.add(kernel)


@pytest.mark.parametrize("mode", [4, 5], ids=["mode4-wavefront", "mode5-team"])
@pytest.mark.parametrize("name", list(ru.ADAPTIVE))
def test_adaptive_factor(name, mode):
    got, log = _decode(name, mode, alpha=0.0)
    _same(got, ru.expected(name, 0.0), f"{name}, mode {mode}, alpha 0")
    _assert_rp(log, ru.kernel_name(ru.CASES[name][0], mode == 5))


def test_all_twelve_instantiations_were_seen():
    """(after test_every_instantiation in file order; it names the kernels itself when run alone)"""
    want = {ru.kernel_name(rung, team) for rung in ru.wu.RUNGS for team in (False, True)}
    assert len(want) == 12
    named = {ru.kernel_name(ru.CASES[name][0], team) for name in ru.CASES for team in (False, True)}
    assert named == want, "the cases name every instantiation"
    if _SEEN:
        assert _SEEN == want, f"not launched: {sorted(want - _SEEN)}"


# ---- 2. the reference's fixtures -----------------------------------------------------------------------------------------------------------
def _same_as_fixture(c, dec, llr, it, cv, rows=None):
    name = c["name"]
    rows = np.ones(len(c["syndromes"]), bool) if rows is None else rows
    dec, llr, it, cv = (_np(x) for x in (dec, llr, it, cv))
    print(f"{name}: decisions differ in {int((dec[rows] != c['decoding'][rows]).any(axis=1).sum())} rows, flags in {int((cv[rows].astype(bool) != c['converge'][rows]).sum())}, "
          f"iterations in {int((it[rows] != c['iterations'][rows]).sum())}, log-ratio checksums in {int((llr_digest(llr)[rows] != c['llr_crc'][rows]).sum())} of {int(rows.sum())}")
    assert np.array_equal(dec[rows], c["decoding"][rows]), "hard decisions differ from the reference's loop"
    assert np.array_equal(cv[rows].astype(bool), c["converge"][rows]), "converge flags differ"
    assert np.array_equal(it[rows], c["iterations"][rows]), "iteration counts differ"
    k = np.flatnonzero(rows[:len(c["llr"])])
    assert bits_equal(llr[k], c["llr"][k]), "log-ratios (rows stored in full) are not the reference's bits"
    assert np.array_equal(llr_digest(llr)[rows], c["llr_crc"][rows]), "log-ratio bit patterns differ in some row"


def _fixture_kernels(name):
    return {ru.kernel_name(ru.FIXTURE_RUNG[name], team) for team in (False, True)}


@pytest.mark.parametrize("mode", [3, 4, 5])
@pytest.mark.parametrize("name", list(ru.FIXTURE_RUNG))
def test_fixtures_c_abi(name, mode):
    """The reference's ``update_channel_probs(P[b]); decode(S[b])`` loop through the synchronous and the asynchronous C entry points; the OSD
    fixtures through ldpc_hip_bposd0_decode_batch_priors[_async]."""
    import torch
    c = ru.load_fixture(name)
    eng = _engine(c["h"], np.full(c["n"], c["own_p"]), c["max_iter"], c["ms_scaling_factor"], c["bp_method"], mode=mode)
    try:
        with launch_util.launch_log() as log:
            out = eng.decode_batch(c["syndromes"], osd0=c["osd"], channel_probs=c["probs"])
        _same_as_fixture(c, *out, rows=ran_bp(c))  # (the C ABI runs BP on an all-zero syndrome too; the fixture holds the reference's shortcut for it)
        ran = launch_util.of(log, ru.RP_KERNEL)
        assert len(ran) == 1 and ran[0] in _fixture_kernels(name) and (mode == 3 or ran[0] == ru.kernel_name(ru.FIXTURE_RUNG[name], mode == 5)), sorted(log)
        _assert_rp(log, ran[0])
        s, p = torch.from_numpy(c["syndromes"].copy()).cuda(), torch.from_numpy(c["probs"].copy()).cuda()
        with launch_util.launch_log() as log:
            out = eng.decode_batch(s, osd0=c["osd"], channel_probs=p, asynchronous=True)
            torch.cuda.synchronize()
        _same_as_fixture(c, *out, rows=ran_bp(c))
        _assert_rp(log, ran[0])
    finally:
        eng.close()


def _decoder(c, **kw):
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    args = dict(error_rate=c["own_p"], max_iter=c["max_iter"], bp_method=c["bp_method"], ms_scaling_factor=c["ms_scaling_factor"], **kw)
    return BpOsdDecoder(c["h"], osd_method="osd_0", **args) if c["osd"] else BpDecoder(c["h"], input_vector_type="syndrome", **args)


@pytest.mark.parametrize("mode", [3, 4, 5])
@pytest.mark.parametrize("name", list(ru.FIXTURE_RUNG))
def test_fixtures_python_api(name, mode):
    """The decoder classes (the ctypes binding, whose engine takes the small-code kernel mode); every row, the all-zero one by the reference's shortcut."""
    c = ru.load_fixture(name)
    d = _decoder(c, _backend="ctypes")
    d._get_engine().set_small_code_kernel(mode)
    with launch_util.launch_log() as log:
        dec = d.decode_batch(c["syndromes"], channel_probs=c["probs"])
    _same_as_fixture(c, dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch)
    ran = launch_util.of(log, ru.RP_KERNEL)
    assert len(ran) == 1 and ran[0] in _fixture_kernels(name), sorted(log)
    assert d.row_prior_route == ("bp_wave_team" if ran[0].endswith(", true>") else "bp_wave")
    assert np.array_equal(d.channel_probs, np.full(c["n"], c["own_p"])), "the decoder's own probabilities must stay"


# ---- 3. beyond the slot kernel ------------------------------------------------------------------------------------------------------------
def test_beyond_the_slot_kernel():
    """hgp1600: one slot of the slot kernel needs 181 328 B.  Default mode: with WAVE_RP = 1 a team per syndrome, with WAVE_RP = 0 the
    per-pass kernels -- the same bits."""
    c = ru.case("hgp1600")
    eng = _engine(c["h"], c["own"], ru.MAX_ITER, ru.ALPHA, switches={"WAVE_RP": 1})
    try:
        assert eng.row_prior_route(ru.BATCH) == "bp_wave_team"
        with launch_util.launch_log() as log:
            on = eng.decode_batch(c["synd"], channel_probs=c["probs"])
        _same(on, ru.expected("hgp1600"), "hgp1600, WAVE_RP = 1")
        _assert_rp(log, "bp_wave_rp_kernel<8, 4, true>")
        eng.set_debug_switch("WAVE_RP", 0)
        assert eng.row_prior_route(ru.BATCH) == "per_pass"
        with launch_util.launch_log() as log:
            off = eng.decode_batch(c["synd"], channel_probs=c["probs"])
        _same(off, ru.expected("hgp1600"), "hgp1600, WAVE_RP = 0")
        assert _route_of(log) == "per_pass"
        _same(off, tuple(_np(x) for x in on), "hgp1600, WAVE_RP = 0 against WAVE_RP = 1")
    finally:
        eng.close()


# ---- 4. work distribution ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [3, 4, 5])
@pytest.mark.parametrize("batch", [1, 3, 70])
@pytest.mark.parametrize("name", ["surface23", "hgp400", "ldpc128_516"])
def test_small_batches(name, batch, mode):
    """B = 1 and B = 3: static teams under modes 3 and 5 (team g takes syndrome g and row g of the priors); B = 70.  The rows are the LAST
    of the case, special rows 129 and 130 among them."""
    rows = slice(ru.BATCH - batch, ru.BATCH)
    got, log = _decode(name, mode, rows=rows)
    _same(got, tuple(x[rows] for x in ru.expected(name)), f"{name}, rows {rows.start} .. 130, mode {mode}")
    ran = launch_util.of(log, ru.RP_KERNEL)
    assert len(ran) == 1
    _assert_rp(log, ran[0])
    if mode != 3 or batch <= 3:
        assert ran[0] == ru.kernel_name(ru.CASES[name][0], mode != 4), "modes 4 / 5 force the form; a handful of syndromes is a team's"


def _poisoned(b, n, want_llr=True):
    """Output tensors no decode leaves as they are: 0xFF bytes (decisions and flags are 0 / 1, iteration counts positive), NaN."""
    import torch
    return (torch.full((b, n), 0xFF, dtype=torch.uint8, device="cuda"),
            torch.full((b, n), float("nan"), dtype=torch.float64, device="cuda") if want_llr else None,
            torch.full((b,), -1, dtype=torch.int32, device="cuda"), torch.full((b,), 0xFF, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("mode,want_llr", [(4, True), (5, True), (5, False)], ids=["mode4-wavefront", "mode5-team", "mode5-team-nollr"])
@pytest.mark.parametrize("name", ru.POOL_CASES)
def test_work_pools(name, mode, want_llr):
    """20 011 rows drawn by index -- syndromes AND priors with the same index -- from a case's 131 rows, pulled from the work counters by
    wavefronts (mode 4) and by teams (mode 5), into poisoned outputs.  Neighbouring rows of the batch are 37 rows apart in the case, with
    different priors: a wavefront or team that kept its previous row's priors, or took those of its own number, decodes to other bits."""
    import torch
    c = ru.case(name)
    idx = ru.pool_index(ru.BATCH)
    want = tuple(x[idx] for x in ru.expected(name))
    assert want[2].min() >= 1, "the poison must differ from every expected value"
    synd = torch.as_tensor(np.ascontiguousarray(c["synd"][idx]), device="cuda")
    probs = torch.as_tensor(np.ascontiguousarray(c["probs"][idx]), device="cuda")
    eng = _engine(c["h"], c["own"], ru.MAX_ITER, ru.ALPHA, mode=mode)
    try:
        out = _poisoned(ru.POOL_ROWS, c["h"].shape[1], want_llr)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(synd, want_llr=want_llr, out=out, channel_probs=probs)
            torch.cuda.synchronize()
    finally:
        eng.close()
    assert all(g is o for g, o in zip(got, out))
    dec, llr, it, cv = (_np(x) for x in got)
    assert set(np.unique(cv).tolist()) <= {0, 1}, "converge flags that were never written"
    _same((dec, llr, it, cv), want, f"{name} x {ru.POOL_ROWS} rows, mode {mode}", want_llr)
    _assert_rp(log, ru.kernel_name(ru.CASES[name][0], mode == 5))


# ---- 5. routing -----------------------------------------------------------------------------------------------------------------------------
def _restated_route(name, mode, wave_rp, default_on):
    """plan_row_prior_route for a min-sum case of this file: outside both lane = edge ladders, taken by the lane = node plan in every mode."""
    if mode == 0:
        return "per_pass"
    if mode != 2 and (mode in (3, 4, 5) or (default_on if wave_rp is None else wave_rp == 1)):
        return "bp_wave*"
    return "bp_small" if name in ru.SLOT_CASES else "per_pass"


@pytest.mark.parametrize("name", list(ru.CASES))
def test_route_query_equals_the_launch_log(name):
    """Every mode x WAVE_RP unset / 0 / 1 on one handle: the query's answer, what the log shows, the route restated here, and the oracle's bits."""
    c = ru.case(name)
    eng = _engine(c["h"], c["own"], ru.MAX_ITER, ru.ALPHA)
    try:
        default_on = eng.row_prior_route(ru.BATCH) in ("bp_wave", "bp_wave_team")
        for mode in MODES:
            eng.set_small_code_kernel(mode)
            for wave_rp in (None, 0, 1):
                eng.set_debug_switch("WAVE_RP", -1 if wave_rp is None else wave_rp)
                said = eng.row_prior_route(ru.BATCH)
                with launch_util.launch_log() as log:
                    got = eng.decode_batch(c["synd"], channel_probs=c["probs"])
                what = f"{name}, mode {mode}, WAVE_RP {wave_rp}"
                assert said in ROUTES and said == _route_of(log), f"{what}: the query says {said}, the log has {sorted(log)}"
                want = _restated_route(name, mode, wave_rp, default_on)
                assert said == want or (want == "bp_wave*" and said in ("bp_wave", "bp_wave_team")), f"{what}: {said}, expected {want}"
                if mode in (4, 5):
                    assert said == ("bp_wave_team" if mode == 5 else "bp_wave"), what
                _same(got, ru.expected(name), what)
    finally:
        eng.close()


def test_the_default_of_the_measured_rule():
    """Modes -1, 1 and 6 with WAVE_RP unset: the lane = node route IS the default -- it beat the parent's row-prior decode on all three measured
    codes (profiles/row_priors_wave.jsonl); WAVE_RP = 0 gives the slot kernel, or for hgp1600 the per-pass kernels, back."""
    for name, off in (("hgp400", "bp_small"), ("hgp1600", "per_pass")):
        c = ru.case(name)
        eng = _engine(c["h"], c["own"], ru.MAX_ITER, ru.ALPHA)
        try:
            for mode in (-1, 1, 6):
                eng.set_small_code_kernel(mode)
                assert eng.row_prior_route(ru.BATCH) in ("bp_wave", "bp_wave_team"), (name, mode)
                eng.set_debug_switch("WAVE_RP", 0)
                assert eng.row_prior_route(ru.BATCH) == off, (name, mode)
                eng.set_debug_switch("WAVE_RP", -1)
            with launch_util.launch_log() as log:
                got = eng.decode_batch(c["synd"], channel_probs=c["probs"])
            assert _route_of(log) in ("bp_wave", "bp_wave_team")
            _same(got, ru.expected(name), f"{name}, mode 6, WAVE_RP unset")
        finally:
            eng.close()


@pytest.mark.parametrize("mode", [-1, 3, 5])
@pytest.mark.parametrize("name", ["bb288", "ldpc64_58"])
def test_product_sum_never_takes_the_route(name, mode):
    c = ru.case(name)
    eng = _engine(c["h"], c["own"], ru.MAX_ITER, 1.0, "product_sum", mode, {"WAVE_RP": 1})
    try:
        said = eng.row_prior_route(ru.BATCH)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"], channel_probs=c["probs"])
    finally:
        eng.close()
    _same(got, ru.expected_product_sum(name), f"{name}, product-sum, mode {mode}")
    launch_util.assert_not_ran(log, ru.RP_KERNEL, "wave_rp_prior_kernel")
    assert said == _route_of(log) == "bp_small"


@pytest.mark.parametrize("wave_rp", [None, 1])
@pytest.mark.parametrize("case_id", ["edge-R2-m17-percol", "edge8-DC3-R3-m17-percol"])
def test_edge_codes_still_take_the_edge_forms(case_id, wave_rp):
    c = next(c for c in lu.ALL_CASES if c.id == case_id)
    h, own, synd = lu.inputs(case_id)
    eng = _engine(h, own, lu.MAX_ITER, c.alpha, mode=c.mode, switches={} if wave_rp is None else {"WAVE_RP": wave_rp})
    try:
        said = eng.row_prior_route(len(synd))
        with launch_util.launch_log() as log:
            got = eng.decode_batch(synd, channel_probs=eu.row_probs(case_id))
        assert said == _route_of(log) == ("bp_edge" if case_id.startswith("edge-") else "bp_edge8")
        assert launch_util.of(log, *eu.RP_KERNELS) == [eu.rp_kernel_name(c.kernel)]
        _same(got, eu.expected(case_id), case_id)
        eng.set_debug_switch("EDGE_RP", 0)  # an edge code the edge forms are switched off for stays on the slot kernel, WAVE_RP or not
        assert eng.row_prior_route(len(synd)) == "bp_small"
    finally:
        eng.close()


@pytest.mark.parametrize("wave_rp", [None, 1])
def test_irregular600_takes_what_it_took_before(wave_rp):
    """irregular_ldpc_code(600, 300, seed=3, col_weights=2/3/6/8/11): columns of more than 8 entries (10 in this draw), so no lane = node rung
    holds the code, whatever the switch says."""
    c = ru.load_fixture("row_priors_irregular_n600_ms16_a0625")
    assert np.diff(c["h"].tocsc().indptr).max() > 8
    eng = _engine(c["h"], np.full(c["n"], c["own_p"]), c["max_iter"], c["ms_scaling_factor"], c["bp_method"], switches={} if wave_rp is None else {"WAVE_RP": wave_rp})
    try:
        routes = {}
        for mode in MODES:
            eng.set_small_code_kernel(mode)
            said = eng.row_prior_route(len(c["syndromes"]))
            with launch_util.launch_log() as log:
                out = eng.decode_batch(c["syndromes"], channel_probs=c["probs"])
            assert said == _route_of(log), (mode, said, sorted(log))
            routes[mode] = said
            _same_as_fixture(c, *out, rows=ran_bp(c))
    finally:
        eng.close()
    small_fits = ru.small_lds_bytes(c["h"], 1) <= 39 * 1024 + 512
    forced_fits = ru.small_lds_bytes(c["h"], 1) <= ru.SLOT_BUDGET
    assert routes[0] == "per_pass"
    for mode in (-1, 3, 4, 5, 6):
        assert routes[mode] == ("bp_small" if small_fits else "per_pass"), routes
    for mode in (1, 2):
        assert routes[mode] == ("bp_small" if forced_fits else "per_pass"), routes


# ---- 6. the handle is left alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bb288", "ldpc128_516", "hgp1600"])
def test_plain_decodes_around_a_row_prior_decode(name):
    """plain, row priors, plain on one handle (mode 3): the plain decodes are bit-identical and launch bp_wave_kernel as before; rows that all
    hold the handle's own probabilities give the plain decode's bits."""
    from ldpc_amd import _lib
    c = ru.case(name)
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    baseline = held()
    eng = _engine(c["h"], c["own"], ru.MAX_ITER, ru.ALPHA, mode=3)
    try:
        with launch_util.launch_log() as log:
            before = eng.decode_batch(c["synd"])
        plain = launch_util.of(log, *lu.BP_DECODE_KERNELS)
        assert len(plain) == 1 and launch_util.base(plain[0]) == "bp_wave_kernel", sorted(log)
        launch_util.assert_not_ran(log, ru.RP_KERNEL, "wave_rp_prior_kernel")
        with launch_util.launch_log() as log:
            own_rows = eng.decode_batch(c["synd"], channel_probs=np.tile(c["own"], (ru.BATCH, 1)))
        assert len(launch_util.of(log, ru.RP_KERNEL)) == 1
        _assert_rp(log, launch_util.of(log, ru.RP_KERNEL)[0])
        _same(own_rows, before, f"{name}: rows of the handle's own probabilities")
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"], channel_probs=c["probs"])
        _assert_rp(log, launch_util.of(log, ru.RP_KERNEL)[0])
        _same(got, ru.expected(name), f"{name}: row priors")
        during = held()
        with launch_util.launch_log() as log:
            after = eng.decode_batch(c["synd"])
        assert launch_util.of(log, *lu.BP_DECODE_KERNELS) == plain, sorted(log)
        launch_util.assert_not_ran(log, ru.RP_KERNEL, "wave_rp_prior_kernel")
        _same(after, before, f"{name}: plain decode after the row-prior decodes")
    finally:
        eng.close()
    n_pad = (c["h"].shape[1] + 63) // 64 * 64
    print(f"{name}: device buffer bytes before {baseline}, with the engine {during}, after close {held()}")
    assert during >= baseline + ru.BATCH * (n_pad + 2) * 8, "the decode went through no counted buffer for the rows' padded log-ratios"
    assert held() == baseline, f"{held() - baseline} bytes of device buffers outlive the handle"


def test_the_decoders_own_probabilities_stay():
    from ldpc_amd.bp_decoder import BpDecoder
    c = ru.case("ldpc64_58")
    d = BpDecoder(c["h"], error_channel=c["own"], max_iter=ru.MAX_ITER, bp_method="minimum_sum", ms_scaling_factor=ru.ALPHA, input_vector_type="syndrome", _backend="ctypes")
    d._get_engine().set_small_code_kernel(3)
    rows = c["synd"].any(axis=1)  # (an all-zero syndrome takes the Python API's shortcut, the reference's)
    with launch_util.launch_log() as log:
        d.decode_batch(c["synd"][rows], channel_probs=c["probs"][rows])
    assert len(launch_util.of(log, ru.RP_KERNEL)) == 1
    want = ru.expected("ldpc64_58")
    assert np.array_equal(d.converge_batch, want[3][rows]) and np.array_equal(d.iter_batch, want[2][rows]) and bits_equal(d.log_prob_ratios_batch, want[1][rows])
    assert np.array_equal(d.channel_probs, c["own"]), "channel_probs of the decoder are unchanged"


# ---- 7. the query through every layer -----------------------------------------------------------------------------------------------------
def test_query_through_every_layer():
    from ldpc_amd import _lib
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    from ldpc_amd.engine import HipBpEngine
    lib = _lib.load()
    assert "ldpc_hip_bp_row_prior_route" in _lib.SYMBOLS and hasattr(lib, "ldpc_hip_bp_row_prior_route")
    assert HipBpEngine.ROW_PRIOR_ROUTES == ROUTES
    c = ru.case("hgp400")
    kw = dict(error_rate=float(c["own"][0]), max_iter=ru.MAX_ITER, bp_method="minimum_sum", ms_scaling_factor=ru.ALPHA)  # (own: p on every bit)
    for d in (BpDecoder(c["h"], input_vector_type="syndrome", **kw), BpOsdDecoder(c["h"], osd_method="osd_0", **kw)):
        assert d.row_prior_route in ROUTES
        eng = d._get_engine()
        assert d.row_prior_route == eng.row_prior_route(1) == eng.row_prior_route(1, want_llr=False)
        eng.set_small_code_kernel(4)
        assert d.row_prior_route == "bp_wave"
        eng.set_small_code_kernel(5)
        assert d.row_prior_route == "bp_wave_team"
        eng.set_small_code_kernel(0)
        assert d.row_prior_route == "per_pass"
        eng.set_small_code_kernel(2)
        assert d.row_prior_route == "bp_small"
    # the batch size last decoded: a handful of syndromes is a team's, a large batch of a code with room for many wavefronts is not
    c = ru.case("ldpc64_58")
    d = BpDecoder(c["h"], input_vector_type="syndrome", _backend="ctypes", **{**kw, "error_rate": float(c["own"][0])})
    d._get_engine().set_small_code_kernel(3)
    assert d.row_prior_route == "bp_wave_team"
    idx = ru.pool_index(ru.BATCH)
    d.decode_batch(np.ascontiguousarray(c["synd"][idx]), channel_probs=np.ascontiguousarray(c["probs"][idx]))
    assert d.row_prior_route == d._get_engine().row_prior_route(ru.POOL_ROWS) == "bp_wave"


def test_query_refusals():
    """Where a row-prior decode is refused, the query raises that decode's NotImplementedError."""
    from ldpc_amd.bp_decoder import BpDecoder
    c = ru.case("ldpc64_58")
    kw = dict(error_rate=float(c["own"][0]), max_iter=ru.MAX_ITER, bp_method="minimum_sum", ms_scaling_factor=ru.ALPHA, input_vector_type="syndrome")

    def refusal_of_a_decode(d):
        with pytest.raises(NotImplementedError) as e:
            d.decode_batch(c["synd"], channel_probs=c["probs"])
        return str(e.value)

    for setup in (dict(schedule="serial"), dict(message_dtype="float32"), dict(memory_strength=0.25), dict(relay=True), dict(decimation=True)):
        d = BpDecoder(c["h"], **{**kw, **{k: v for k, v in setup.items() if k == "schedule"}})
        if "message_dtype" in setup:
            d.message_dtype = "float32"
        if "memory_strength" in setup:
            d.memory_strength = 0.25
        if "relay" in setup:
            d.relay = dict(pre_iter=4, num_sets=2, set_max_iter=4)
        if "decimation" in setup:
            d.decimation = dict(round_iters=4, max_rounds=3)
        with pytest.raises(NotImplementedError) as e:
            d.row_prior_route
        assert str(e.value) == refusal_of_a_decode(d), setup
    d = BpDecoder(c["h"], device_ids=[0], **kw)
    with pytest.raises(NotImplementedError, match="device_ids"):
        d.row_prior_route
    # the engine: the library's own refusal
    eng = _engine(c["h"], c["own"], ru.MAX_ITER, ru.ALPHA)
    try:
        eng.set_message_dtype("float32")
        with pytest.raises(NotImplementedError, match="float32 messages: per-row channel probabilities are not available"):
            eng.row_prior_route(4)
        eng.set_message_dtype("float64")
        eng.set_memory(np.full(c["h"].shape[1], 0.25))
        with pytest.raises(NotImplementedError, match="memory min-sum: per-row channel probabilities are not available"):
            eng.row_prior_route(4)
        eng.set_memory(None)
        assert eng.row_prior_route(4) in ROUTES
        with pytest.raises(Exception):
            eng.row_prior_route(-1)
    finally:
        eng.close()
