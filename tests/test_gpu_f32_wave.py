"""The float32 message mode on the lane = node kernel (ldpc_amd/csrc/bp_wave_f32_kernel.h; opt-in: ldpc_hip_bp_set_f32_lane_node) against the
NumPy restatement (tests/f32_util.py) -- hard decisions, iteration counts, converge flags and the bit patterns of the log-ratios -- on a
smallest code for every instantiation (tests/f32_wave_util.py; tests/test_f32_wave_cases.py checks the cases without a GPU), in both forms
of the log-ratios and without them, the launch log showing that exactly the named instantiation ran.  With the switch off the same cases
take the per-pass kernels and give the same bits.  Then the routing order, the work counters on 20 011 rows, special values, and what goes
round the kernel: a handle that changes its dtype and its priors, BpDecoder and BpOsdDecoder on both backends, the b8 entry points, what
float32 refuses, close(), and the three new C entry points on invalid arguments."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import f32_onchip_util as ou
import f32_util as fu
import f32_wave_util as wu
import ladder_util as lu
import launch_util
from oracle import bits_equal

pytestmark = pytest.mark.gpu

POOL_ROWS = 20011
IDS = [c.id for c in wu.CASES]


def _same(got, want, what, llr=True):
    dec, gl, it, cv = got
    print(f"{what}: {int(np.count_nonzero(np.asarray(dec) != want[0]))} decisions, {int(np.count_nonzero(np.asarray(cv, bool) != want[3]))} flags, "
          f"{int(np.count_nonzero(np.asarray(it) != want[2]))} iteration counts differ")
    assert np.array_equal(np.asarray(dec), want[0]), f"{what}: hard decisions"
    assert np.array_equal(np.asarray(cv, bool), want[3]), f"{what}: converge flags"
    assert np.array_equal(np.asarray(it), want[2]), f"{what}: iteration counts"
    if not llr:
        assert gl is None
        return
    gl = np.asarray(gl)
    assert bits_equal(gl, want[1]), f"{what}: log-ratios differ in some bit"
    assert np.array_equal(gl, gl.astype(np.float32).astype(np.float64), equal_nan=True), f"{what}: a log-ratio that is no widened float32"


def _shortcut(want, synd):
    """What BpDecoder.decode_batch reports: all-zero rows take the host shortcut (zeros, converged, 0 iterations)."""
    dec, llr, it, cv = (x.copy() for x in want)
    zero = ~synd.any(axis=1)
    dec[zero], llr[zero], it[zero], cv[zero] = 0, 0.0, 0, True
    return dec, llr, it, cv


def _engine(c, mode=None, switches=None, dtype="float32", method=1, lane_node=True):
    from ldpc_amd.engine import HipBpEngine
    h = sp.csr_matrix(c["h"])
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], c["probs"], c["max_iter"], method, c["alpha"])
    eng.set_message_dtype(dtype)
    if lane_node:
        eng.set_f32_lane_node(True)
    if mode is not None:
        eng.set_small_code_kernel(mode)
    for name, value in (switches or {}).items():
        eng.set_debug_switch(name, value)
    return eng


def _decode(c, mode=None, switches=None, lane_node=True, route=None, **kw):
    eng = _engine(c, mode, switches, lane_node=lane_node)
    try:
        if route is not None:
            assert eng.f32_route(len(c["synd"]), kw.get("want_llr", True)) == route
        with launch_util.launch_log() as log:
            out = eng.decode_batch(c["synd"], **kw)
    finally:
        eng.close()
    return out, log


def _assert_wave(log, name):
    """Exactly the named instantiation, once; no per-pass float32 kernel, no lane = edge float32 kernel and no FP64 decode kernel."""
    launch_util.assert_resolved(log)
    assert launch_util.of(log, *wu.ONCHIP_WAVE) == [name], f"expected exactly {name}; the log has {sorted(log)}"
    assert log[name] == 1
    launch_util.assert_not_ran(log, *wu.PER_PASS, *wu.ONCHIP_EDGE, *lu.BP_DECODE_KERNELS)


def _assert_per_pass(log):
    launch_util.assert_ran(log, *wu.PER_PASS)
    launch_util.assert_not_ran(log, *wu.ONCHIP_WAVE, *wu.ONCHIP_EDGE, *(k for k in lu.BP_DECODE_KERNELS if k not in wu.PER_PASS))


# ---- 1. every instantiation, in both forms of the log-ratios and without them ----------------------------------------------------------------
@pytest.mark.parametrize("form", ["llr-copy", "llr-direct", "no-llr"])
@pytest.mark.parametrize("case_id", IDS)
def test_every_instantiation(case_id, form):
    case = wu.BY_ID[case_id]
    switches = {"llr-copy": {"F32_WAVE_LLR": 0}, "llr-direct": {"F32_WAVE_LLR": 1}, "no-llr": {}}[form]
    got, log = _decode(wu.case_dict(case_id), case.mode, switches, route=wu.route_name(case.team), want_llr=form != "no-llr")
    _same(got, wu.expected(case_id), f"{case_id}/{form}", llr=form != "no-llr")
    _assert_wave(log, wu.kernel_name(case.dr, case.dc, case.team))


# ---- 2. switch off: today's routing, the same bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", IDS)
def test_switch_off_takes_the_per_pass_kernels(case_id):
    case = wu.BY_ID[case_id]
    got, log = _decode(wu.case_dict(case_id), case.mode, lane_node=False, route="per_pass")
    _same(got, wu.expected(case_id), f"{case_id} with the switch off")
    _assert_per_pass(log)


def test_the_switch_is_off_by_default():
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    c = wu.case_dict(wu.DEFAULT_MODE_CASE)
    eng = _engine(c, lane_node=False)
    try:
        assert eng.f32_lane_node is False and eng.f32_route(131) == "per_pass"
        eng.set_f32_lane_node(True)
        assert eng.f32_lane_node is True and eng.f32_route(131) == "bp_wave_team"
        eng.set_message_dtype("float64")  # (the route answers for a float32 decode whatever the dtype is now)
        assert eng.f32_route(131) == "bp_wave_team"
        eng.set_f32_lane_node(False)
        assert eng.f32_lane_node is False and eng.f32_route(131) == "per_pass"
    finally:
        eng.close()
    for cls in (BpDecoder, BpOsdDecoder):
        d = cls(c["h"], error_rate=0.04, max_iter=8, bp_method="minimum_sum")
        assert d.float32_lane_node is False and d.message_dtype == "float64"
        d.float32_lane_node = True  # (no particular dtype is required)
        assert d.float32_lane_node is True
        with pytest.raises(ValueError):
            d.float32_lane_node = 1


# ---- 3. routing order with the switch on -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["edge-R2-m17-percol", "edge8-DC3-R3-m17-percol"])
def test_lane_edge_codes_keep_their_kernels(case_id):
    case = next(c for c in ou.ONCHIP_CASES if c.id == case_id)
    name = ou.f32_kernel_name(case.kernel)
    got, log = _decode(ou.case_dict(case_id), -1, route="bp_edge8" if "edge8" in name else "bp_edge")
    _same(got, ou.expected(case_id), f"{case_id} under mode -1 with the switch on")
    assert launch_util.of(log, *wu.ONCHIP_EDGE) == [name] and log[name] == 1
    launch_util.assert_not_ran(log, *wu.ONCHIP_WAVE, *wu.PER_PASS)


@pytest.mark.parametrize("how", ["mode 6", "mode 0", "mode 2", "F32_ONCHIP=0", "F32_NT=0"])
def test_what_keeps_a_wave_only_code_per_pass(how):
    mode, switches = {"mode 6": (6, {}), "mode 0": (0, {}), "mode 2": (2, {}), "F32_ONCHIP=0": (-1, {"F32_ONCHIP": 0}), "F32_NT=0": (-1, {"F32_NT": 0})}[how]
    got, log = _decode(wu.case_dict(wu.DEFAULT_MODE_CASE), mode, switches, route="per_pass")
    _same(got, wu.expected(wu.DEFAULT_MODE_CASE), f"{wu.DEFAULT_MODE_CASE} with {how}")
    _assert_per_pass(log)


@pytest.mark.parametrize("mode,team", [(4, False), (5, True), (3, True), (1, True)])
def test_modes_force_the_form(mode, team):
    """4 and 5 force one wavefront and a team; 3 and 1 take the plan's choice, which for 131 syndromes is the team."""
    got, log = _decode(wu.case_dict(wu.DEFAULT_MODE_CASE), mode, route=wu.route_name(team))
    _same(got, wu.expected(wu.DEFAULT_MODE_CASE), f"{wu.DEFAULT_MODE_CASE} under mode {mode}")
    _assert_wave(log, wu.kernel_name(16, 8, team))


def test_a_code_with_an_empty_column():
    """The lane = edge families decline a column without entries (no lane would write its outputs); the lane = node layout has a lane per
    column whatever its weight.  With the switch off such a code goes per-pass, as ever."""
    c = fu.degree1_case()
    h = sp.csr_matrix(c["h"])
    assert int(np.asarray(h.sum(axis=0)).min()) == 0 and len(c["synd"]) <= 256
    dr, dc = wu.rung_of(int(np.diff(h.indptr).max()), int(np.bincount(h.indices, minlength=h.shape[1]).max()))
    want = fu.expected("degree1_empty", c, np.float32)
    got, log = _decode(c, -1, route="bp_wave_team")  # (no more syndromes than 256 wavefront slots: a team each)
    _same(got, want, "degree1_empty with the switch on")
    _assert_wave(log, wu.kernel_name(dr, dc, True))
    got, log = _decode(c, -1, lane_node=False, route="per_pass")
    _same(got, want, "degree1_empty with the switch off")
    _assert_per_pass(log)


# ---- 4. the work counters ----------------------------------------------------------------------------------------------------------------------
def _poisoned(b, n, want_llr=True):
    """Output tensors no decode leaves as they are: 0xFF bytes (decisions and flags are 0 / 1, iteration counts positive), NaN."""
    import torch
    return (torch.full((b, n), 0xFF, dtype=torch.uint8, device="cuda"),
            torch.full((b, n), float("nan"), dtype=torch.float64, device="cuda") if want_llr else None,
            torch.full((b,), -1, dtype=torch.int32, device="cuda"), torch.full((b,), 0xFF, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("rows", [POOL_ROWS, 1, 2])
@pytest.mark.parametrize("case_id", ["wave_f32-8x4-mode4", "wave_f32-6x3-mode5"])
def test_work_counters(case_id, rows):
    """20 011 rows drawn by index from a case's rows (rows are independent), into poisoned outputs -- a row nobody decodes shows as missing,
    not as stale: lone wavefronts pull from the pooled counters, teams from the first counter.  Teams are assigned statically only while
    there are no more syndromes than resident teams, 256 compute units x the teams of one -- at most eight, sixteen wavefronts in all and two
    a team at least: 20 011 is beyond that.  One and two rows: the static path of the teams, a pool of one or two for the lone wavefronts."""
    import torch
    case = wu.BY_ID[case_id]
    c, want_rows = wu.case_dict(case_id), wu.expected(case_id)
    idx = (np.arange(rows, dtype=np.int64) * 37 + 1) % len(c["synd"])
    want = tuple(x[idx] for x in want_rows)
    assert not np.isnan(want[1]).any() and want[2].min() >= 1, "the poison must differ from every expected value"
    synd = torch.as_tensor(np.ascontiguousarray(c["synd"][idx]), device="cuda")
    eng = _engine(c, case.mode)
    try:
        assert eng.f32_route(rows) == wu.route_name(case.team)
        static_bound = 256 * (16 // 2)
        assert (rows > static_bound) == (rows == POOL_ROWS)
        out = _poisoned(rows, want[0].shape[1])
        with launch_util.launch_log() as log:
            got = eng.decode_batch(synd, out=out)
            torch.cuda.synchronize()
    finally:
        eng.close()
    assert all(g is o for g, o in zip(got, out))
    dec, llr, it, cv = (x.cpu().numpy() for x in got)
    assert set(np.unique(cv).tolist()) <= {0, 1}, "converge flags that were never written"
    _same((dec, llr, it, cv), want, f"{case_id} x {rows} rows")
    _assert_wave(log, wu.kernel_name(case.dr, case.dc, case.team))


# ---- 5. special values -------------------------------------------------------------------------------------------------------------------------
# hamming_code(3): 3 rows of 4, columns of up to 3 entries -- rung (4,4).  rep_code(5): 4 rows of 2, columns of up to 2 -- rung (4,2).
_SPECIAL_RUNG = {"hamming3": (4, 4), "rep5": (4, 2)}


@pytest.mark.parametrize("mode", [4, 5])
@pytest.mark.parametrize("alpha", [0.625, 1.0, 0.0])
@pytest.mark.parametrize("code", ["hamming3", "rep5"])
def test_special_values(code, alpha, mode):
    """Priors of +-inf and 0, p = 1e-300, syndrome bytes 2 and 3 and an all-zero row, through the engine (no host shortcut)."""
    c = fu.small_case(code, alpha)
    got, log = _decode(c, mode, route=wu.route_name(mode == 5))
    _same(got, fu.expected(f"{code}_a{alpha}", c, np.float32), f"{code} a = {alpha} mode {mode}")
    _assert_wave(log, wu.kernel_name(*_SPECIAL_RUNG[code], mode == 5))


# ---- 6. around the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["wave_f32-4x4-mode5", "wave_f32-8x4-mode4"])
def test_dtype_round_trip(case_id, oracle_built):
    """float32, float64, float32, float64 on one handle with the switch on: the position tables are shared, each dtype writes its own padded
    priors before every launch -- neither may read the other's.  FP64 decodes on bp_wave_kernel and equals the oracle.  (The team case has
    per-column priors, the one-wavefront case one prior for all columns: ladder_util draws them so.)"""
    case = wu.BY_ID[case_id]
    ladder = next(c for c in lu.WAVE_CASES if c.id == case.ladder)
    assert ladder.uniform == (case.mode == 4)
    c = wu.case_dict(case_id)
    eng = _engine(c, case.mode)
    try:
        for dtype in ("float32", "float64", "float32", "float64"):
            eng.set_message_dtype(dtype)
            with launch_util.launch_log() as log:
                got = eng.decode_batch(c["synd"])
            if dtype == "float32":
                _same(got, wu.expected(case_id), f"{case_id} in float32")
                _assert_wave(log, wu.kernel_name(case.dr, case.dc, case.team))
            else:
                want = lu.expected(case.ladder)
                for k, name in ((0, "decoding"), (2, "iterations"), (3, "converge")):
                    assert np.array_equal(got[k], np.asarray(want[k]).astype(got[k].dtype)), f"{case_id} in float64: {name}"
                assert bits_equal(got[1], np.asarray(want[1])), f"{case_id} in float64: log-ratios"
                assert launch_util.of(log, *lu.BP_DECODE_KERNELS) == [ladder.kernel] and log[ladder.kernel] == 1, sorted(log)
                launch_util.assert_not_ran(log, *wu.ONCHIP_WAVE)
    finally:
        eng.close()


def test_set_channel_is_followed():
    case_id = "wave_f32-6x3-mode4"
    case = wu.BY_ID[case_id]
    c = wu.case_dict(case_id)
    other = np.clip(np.asarray(c["probs"])[::-1] * 1.5, 0.0, 0.9)
    assert not np.array_equal(other, c["probs"])
    want_other = fu.min_sum_restatement(c["h"], other, c["synd"], c["max_iter"], c["alpha"], np.float32)
    assert not bits_equal(want_other[1], wu.expected(case_id)[1])
    eng = _engine(c, case.mode)
    try:
        _same(eng.decode_batch(c["synd"]), wu.expected(case_id), f"{case_id} before set_channel")
        eng.set_channel(other)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, want_other, f"{case_id} after set_channel")
        _assert_wave(log, wu.kernel_name(case.dr, case.dc, case.team))
    finally:
        eng.close()


def _decoder(c, backend=None, cls=None, lane_node=True, **kw):
    from ldpc_amd.bp_decoder import BpDecoder
    d = (cls or BpDecoder)(c["h"], error_channel=list(c["probs"]), max_iter=c["max_iter"], bp_method="minimum_sum",
                           ms_scaling_factor=c["alpha"], input_vector_type="syndrome", **({"_backend": backend} if backend else {}), **kw)
    d.message_dtype = "float32"
    d.float32_lane_node = lane_node
    return d


@pytest.mark.parametrize("backend", ["cython", "ctypes"])
def test_bp_decoder(backend):
    """decode_batch and decode() of BpDecoder on both backends (the decoder classes run under the default small-code kernel mode)."""
    case_id = wu.DEFAULT_MODE_CASE
    c, want = wu.case_dict(case_id), wu.expected(case_id)
    d = _decoder(c, backend)
    with launch_util.launch_log() as log:
        dec = d.decode_batch(c["synd"])
    _same((dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), _shortcut(want, c["synd"]), f"{case_id}/decode_batch/{backend}")
    _assert_wave(log, wu.kernel_name(16, 8, True))
    assert d.float32_route == "bp_wave_team"
    for row in (int(np.flatnonzero(want[3] & c["synd"].any(axis=1))[0]), int(np.flatnonzero(~want[3])[0])):
        with launch_util.launch_log() as log:
            out = d.decode(c["synd"][row])
        _same((out[None, :], d.log_prob_ratios[None, :], np.array([d.iter]), np.array([d.converge])), tuple(x[row:row + 1] for x in want),
              f"{case_id}/decode row {row}/{backend}")
        _assert_wave(log, wu.kernel_name(16, 8, True))
    d.float32_lane_node = False
    with launch_util.launch_log() as log:
        dec = d.decode_batch(c["synd"])
    _same((dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), _shortcut(want, c["synd"]), f"{case_id}/switched off again/{backend}")
    _assert_per_pass(log)
    assert d.float32_route == "per_pass"


@pytest.mark.parametrize("osd_method,osd_order,code", [("osd_0", 0, 1), ("osd_cs", 4, 3)])
def test_bposd_switch_on_against_off(osd_method, osd_order, code):
    """OSD sees the same widened posteriors from either route: identical decisions, outputs and OSD status bytes."""
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    case_id = wu.DEFAULT_MODE_CASE
    c, want = wu.case_dict(case_id), wu.expected(case_id)
    assert int((~want[3]).sum()) >= 10
    results = {}
    for on in (True, False):
        eng = _engine(c, lane_node=on)
        try:
            eng.set_osd(code, osd_order)
            with launch_util.launch_log() as log:
                got = eng.decode_batch(c["synd"], osd=True)
            results[on] = tuple(np.array(x) for x in got) + (eng.osd_status(len(c["synd"])),)
        finally:
            eng.close()
        (_assert_wave(log, wu.kernel_name(16, 8, True)) if on else _assert_per_pass(log))
    for k, name in enumerate(("decoding", "log-ratios", "iterations", "converge", "OSD status")):
        assert (bits_equal(results[True][k], results[False][k]) if k == 1 else np.array_equal(results[True][k], results[False][k])), f"{osd_method}: {name}"
    status = results[True][4]
    assert np.array_equal(status == 0, want[3]) and (status > 0).any(), "status 0 exactly where BP converged"
    assert np.array_equal(results[True][0][want[3]], want[0][want[3]]) and bits_equal(results[True][1], want[1])
    for backend in ("cython", "ctypes"):
        outs = []
        for on in (True, False):
            d = _decoder(c, backend, cls=BpOsdDecoder, lane_node=on, osd_method=osd_method, osd_order=osd_order)
            outs.append(np.array(d.decode_batch(c["synd"])))
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], _shortcut(results[True][:4], c["synd"])[0]), f"BpOsdDecoder/{osd_method}/{backend}"


def test_b8_entry_points_switch_on_against_off():
    """decode_b8 and simulate_b8 (fixed seed) on a detector error model beyond the lane = edge families: identical outputs and counts."""
    from test_gpu_dem_sampler import SEED, engine, model, twin
    check, obs, pri = model("bb144x3")
    _, dets, _ = twin("bb144x3", False, 0)
    results = {}
    for on in (True, False):
        eng = engine(check, pri, obs)
        try:
            eng.set_message_dtype("float32")
            eng.set_f32_lane_node(on)
            eng.set_osd(1, 0)
            assert eng.f32_route(3000, False) in (("bp_wave", "bp_wave_team") if on else ("per_pass",))
            with launch_util.launch_log() as log:
                b8 = [eng.decode_b8(np.array(dets), with_osd=w, want_decoding=True) for w in (False, True)]
                sim = eng.simulate_b8(SEED, 0, 3000, chunk=1024, with_osd=True)
            results[on] = ([tuple(np.array(x) for x in r) for r in b8], tuple(int(v) for v in sim))
        finally:
            eng.close()
        if on:
            launch_util.assert_ran(log, "bp_wave_f32_kernel")
            launch_util.assert_not_ran(log, *wu.PER_PASS)
        else:
            _assert_per_pass(log)
    for r_on, r_off in zip(results[True][0], results[False][0]):
        for a, b in zip(r_on, r_off):
            assert np.array_equal(a, b), "decode_b8: switch on against off"
    assert results[True][1] == results[False][1], f"simulate_b8: {results[True][1]} with the switch on, {results[False][1]} with it off"
    print(f"bb144x3 float32 + OSD-0, 3000 shots: (logical failures, rows BP left unconverged) = {results[True][1]} on either route")


def test_monte_carlo_dem_simulation_carries_the_switch():
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from test_gpu_dem_sampler import SEED, model
    runs = []
    for on in (True, False):
        sim = MonteCarloDemSimulation(model("bb144x3"), target_run_count=2048, batch_size=1024, seed=SEED, max_iter=12, message_dtype="float32", float32_lane_node=on)
        with launch_util.launch_log() as log:
            out = sim.run()
        runs.append((out["fail_count"], out["bp_unconverged_count"]))
        (launch_util.assert_ran(log, "bp_wave_f32_kernel") if on else _assert_per_pass(log))
    assert runs[0] == runs[1]
    with pytest.raises(ValueError):
        MonteCarloDemSimulation(model("bb144x3"), target_run_count=1, float32_lane_node=1)


def test_refusals_stand_with_the_switch_on():
    from ldpc_amd import _lib
    case_id = wu.DEFAULT_MODE_CASE
    c = wu.case_dict(case_id)
    n = c["h"].shape[1]
    eng = _engine(c, method=0)  # product-sum
    try:
        with pytest.raises(_lib.LdpcHipError, match=r"error -4: float32 messages: product-sum"):
            eng.decode_batch(c["synd"])
        eng.set_params(c["max_iter"], 1, c["alpha"])
        eng.set_schedule("serial")
        with pytest.raises(_lib.LdpcHipError, match=r"error -4: float32 messages: the serial schedules"):
            eng.decode_batch(c["synd"])
        eng.set_schedule("parallel")
        for osd0 in (False, True):
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: float32 messages: per-row channel probabilities"):
                eng.decode_batch(c["synd"], osd0=osd0, channel_probs=np.tile(c["probs"], (len(c["synd"]), 1)))
        eng.set_memory(np.full(n, 0.25))
        with pytest.raises(_lib.LdpcHipError, match=r"error -4: .*float32"):
            eng.decode_batch(c["synd"])
        eng.set_memory(None)
        eng.set_relay(np.full((2, n), 0.25), [4, 4], 1)
        with pytest.raises(_lib.LdpcHipError, match=r"error -4: .*float32"):
            eng.decode_batch(c["synd"])
        eng.set_relay(None)
        eng.set_decimation(3, 4, 25.0)
        with pytest.raises(_lib.LdpcHipError, match=r"error -4: .*float32"):
            eng.decode_batch(c["synd"])
        eng.set_decimation(None)
        with launch_util.launch_log() as log:  # ... and the handle still decodes, on chip
            got = eng.decode_batch(c["synd"])
        _same(got, wu.expected(case_id), f"{case_id} after the refusals")
        _assert_wave(log, wu.kernel_name(16, 8, True))
    finally:
        eng.close()


def test_close_frees_every_device_buffer():
    from ldpc_amd import _lib
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    for case_id in ("wave_f32-8x8-mode4", wu.DEFAULT_MODE_CASE):
        c = wu.case_dict(case_id)
        eng = _engine(c, wu.BY_ID[case_id].mode)
        try:
            eng.decode_batch(c["synd"])
            with_priors = held()
            eng.set_f32_lane_node(False)  # (the padded float32 priors go with the route)
            assert held() < with_priors
            eng.set_f32_lane_node(True)
            eng.set_message_dtype("float64")
            eng.decode_batch(c["synd"])
            eng.set_message_dtype("float32")
            eng.set_osd(1, 0)
            eng.decode_batch(c["synd"], osd=True)
            during = held()
        finally:
            eng.close()
        after = held()
        print(f"float32 lane = node: device buffer bytes before {before}, with the engine {during}, after close {after}")
        assert during > before and after == before, f"{after - before} bytes of device buffers outlive the handle"


# ---- 7. the setter, the getter and the route on invalid arguments ------------------------------------------------------------------------------
def test_the_c_entry_points_on_invalid_arguments():
    from ldpc_amd import _lib
    lib = _lib.load()
    INVALID = -1
    c = wu.case_dict(wu.DEFAULT_MODE_CASE)
    eng = _engine(c, lane_node=False)
    try:
        h = eng._h
        on, route = C.c_int32(7), C.c_int32(7)
        assert lib.ldpc_hip_bp_set_f32_lane_node(None, 1) == INVALID
        for bad in (2, -1, 256):
            assert lib.ldpc_hip_bp_set_f32_lane_node(h, bad) == INVALID
            assert b"0 or 1" in lib.ldpc_hip_last_error()
        assert lib.ldpc_hip_bp_get_f32_lane_node(None, C.byref(on)) == INVALID and lib.ldpc_hip_bp_get_f32_lane_node(h, None) == INVALID
        assert lib.ldpc_hip_bp_get_f32_lane_node(h, C.byref(on)) == 0 and on.value == 0, "a refused value changes nothing"
        assert lib.ldpc_hip_bp_f32_route(None, 1, 1, C.byref(route)) == INVALID and lib.ldpc_hip_bp_f32_route(h, 1, 1, None) == INVALID
        assert lib.ldpc_hip_bp_f32_route(h, -1, 1, C.byref(route)) == INVALID and route.value == 7
        assert lib.ldpc_hip_bp_f32_route(h, 0, 1, C.byref(route)) == 0 and route.value == 0
        assert lib.ldpc_hip_bp_set_f32_lane_node(h, 1) == 0 and lib.ldpc_hip_bp_get_f32_lane_node(h, C.byref(on)) == 0 and on.value == 1
        assert lib.ldpc_hip_bp_f32_route(h, 131, 1, C.byref(route)) == 0 and route.value == 4
        assert lib.ldpc_hip_bp_f32_route(h, 1 << 30, 1, C.byref(route)) == 0 and route.value == 0, "beyond the work pools' 32-bit syndrome indices: per-pass"
        with pytest.raises(_lib.LdpcHipError):
            eng.set_debug_switch("F32_WAVE_LLR_", 1)
    finally:
        eng.close()
