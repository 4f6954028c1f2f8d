"""The float32 message mode on the codes of the lane = edge families: bp_edge_f32_kernel and bp_edge8_f32_kernel
(ldpc_amd/csrc/bp_edge_f32_kernel.h) against the NumPy restatement (tests/f32_util.py) -- hard decisions, iteration counts, converge flags
and the bit patterns of the log-ratios -- on a smallest code for every instantiation (tests/ladder_util.py; tests/test_f32_onchip_cases.py
checks the cases without a GPU), with the launch log showing that exactly the named float32 instantiation ran.  Just outside the bounds,
with the route switched off, and for every code the planners decline, the per-pass kernels run and give the same bits.  Then what goes
round the kernels: special values, the work pools on 20 011 rows, a handle that changes its dtype back and forth, BpDecoder and
BpOsdDecoder, what the mode refuses, and that close() frees every buffer."""
import numpy as np
import pytest
import scipy.sparse as sp

import f32_onchip_util as ou
import f32_util as fu
import ladder_util as lu
import launch_util
from oracle import bits_equal

pytestmark = pytest.mark.gpu

POOL_ROWS = 20011


def _same(got, want, what):
    dec, llr, it, cv = got
    print(f"{what}: {int(np.count_nonzero(np.asarray(dec) != want[0]))} decisions, {int(np.count_nonzero(np.asarray(cv, bool) != want[3]))} flags, "
          f"{int(np.count_nonzero(np.asarray(it) != want[2]))} iteration counts differ")
    assert np.array_equal(np.asarray(dec), want[0]), f"{what}: hard decisions"
    assert np.array_equal(np.asarray(cv, bool), want[3]), f"{what}: converge flags"
    assert np.array_equal(np.asarray(it), want[2]), f"{what}: iteration counts"
    llr = np.asarray(llr)
    assert bits_equal(llr, want[1]), f"{what}: log-ratios differ in some bit"
    assert np.array_equal(llr, llr.astype(np.float32).astype(np.float64), equal_nan=True), f"{what}: a log-ratio that is no widened float32"


def _shortcut(want, synd):
    """What BpDecoder.decode_batch reports: all-zero rows take the host shortcut (zeros, converged, 0 iterations)."""
    dec, llr, it, cv = (x.copy() for x in want)
    zero = ~synd.any(axis=1)
    dec[zero], llr[zero], it[zero], cv[zero] = 0, 0.0, 0, True
    return dec, llr, it, cv


def _engine(c, mode=None, switches=None, dtype="float32", method=1):
    from ldpc_amd.engine import HipBpEngine
    h = sp.csr_matrix(c["h"])
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], c["probs"], c["max_iter"], method, c["alpha"])
    eng.set_message_dtype(dtype)
    if mode is not None:
        eng.set_small_code_kernel(mode)
    for name, value in (switches or {}).items():
        eng.set_debug_switch(name, value)
    return eng


def _decode(c, mode=None, switches=None, **kw):
    eng = _engine(c, mode, switches)
    try:
        with launch_util.launch_log() as log:
            out = eng.decode_batch(c["synd"], **kw)
    finally:
        eng.close()
    return out, log


def _assert_onchip(log, name):
    """Exactly the named float32 instantiation, once; no per-pass float32 kernel and no FP64 decode kernel."""
    launch_util.assert_resolved(log)
    assert launch_util.of(log, *ou.ONCHIP) == [name], f"expected exactly {name}; the log has {sorted(log)}"
    assert log[name] == 1
    launch_util.assert_not_ran(log, *ou.PER_PASS, *lu.BP_DECODE_KERNELS)


def _assert_per_pass(log):
    launch_util.assert_ran(log, *ou.PER_PASS)
    launch_util.assert_not_ran(log, *ou.ONCHIP, *(k for k in lu.BP_DECODE_KERNELS if k not in ou.PER_PASS))


def _decoder(c, backend=None, cls=None, **kw):
    from ldpc_amd.bp_decoder import BpDecoder
    d = (cls or BpDecoder)(c["h"], error_channel=list(c["probs"]), max_iter=c["max_iter"], bp_method="minimum_sum",
                           ms_scaling_factor=c["alpha"], input_vector_type="syndrome", **({"_backend": backend} if backend else {}), **kw)
    d.message_dtype = "float32"
    return d


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ou.ONCHIP_CASES, ids=[c.id for c in ou.ONCHIP_CASES])
def test_every_instantiation(case):
    got, log = _decode(ou.case_dict(case.id), case.mode, case.switches)
    _same(got, ou.expected(case.id), case.id)
    _assert_onchip(log, ou.f32_kernel_name(case.kernel))


# ---- 2. just outside the bounds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lu.OUTSIDE_CASES, ids=[c.id for c in lu.OUTSIDE_CASES])
def test_just_outside_the_bounds(case):
    got, log = _decode(ou.case_dict(case.id), case.mode, case.switches)
    _same(got, ou.expected(case.id), case.id)
    if case.kernel is None:
        _assert_per_pass(log)
    else:
        assert case.id in ("outside-weight5-row", "outside-weight3-column")
        _assert_onchip(log, "bp_edge8_f32_kernel<5, 3, true>")


# ---- 3. special values -----------------------------------------------------------------------------------------------------------------
# hamming_code(3): 3 rows of 4, columns of up to 3 entries -- no bp_edge code; bp_edge8 with DC 3, 24 slots: the smallest R, 2.
# rep_code(5): 4 rows of 2, columns of up to 2 entries -- bp_edge, 16 slots: R = 1.  Per-column priors: UNIFORM = false (and so no NOCLAMP).
_SPECIAL_KERNEL = {"hamming3": "bp_edge8_f32_kernel<2, 3, false>", "rep5": "bp_edge_f32_kernel<1, false, false>"}


@pytest.mark.parametrize("alpha", [0.625, 1.0, 0.0])
@pytest.mark.parametrize("code", ["hamming3", "rep5"])
def test_special_values(code, alpha):
    """Priors of +-inf and 0, p = 1e-300, syndrome bytes 2 and 3 and an all-zero row, through the engine (no host shortcut)."""
    c = fu.small_case(code, alpha)
    got, log = _decode(c)
    _same(got, fu.expected(f"{code}_a{alpha}", c, np.float32), f"{code} a = {alpha}")
    _assert_onchip(log, _SPECIAL_KERNEL[code])


def test_degree1_case_takes_the_per_pass_route():
    """The fixture has a column without entries: plan_edge and plan_edge8 decline such a code (no lane would write its outputs)."""
    c = fu.degree1_case()
    assert int(np.asarray(sp.csr_matrix(c["h"]).sum(axis=0)).min()) == 0
    got, log = _decode(c)
    _same(got, fu.expected("degree1_empty", c, np.float32), "degree1_empty")
    _assert_per_pass(log)


# ---- 4. work pools and chunks of pulls -----------------------------------------------------------------------------------------------
def _poisoned(b, n, want_llr=True):
    """Output tensors no decode leaves as they are: 0xFF bytes (decisions and flags are 0 / 1, iteration counts positive), NaN."""
    import torch
    return (torch.full((b, n), 0xFF, dtype=torch.uint8, device="cuda"),
            torch.full((b, n), float("nan"), dtype=torch.float64, device="cuda") if want_llr else None,
            torch.full((b,), -1, dtype=torch.int32, device="cuda"), torch.full((b,), 0xFF, dtype=torch.uint8, device="cuda"))


_POOL_CASES = {"edge": ("edge-R1-m16-noclamp", "bp_edge_f32_kernel<1, true, true>"), "bb144": (None, "bp_edge8_f32_kernel<9, 3, true>")}


def _pool_case(key):
    case_id, kernel = _POOL_CASES[key]
    if case_id:
        return ou.case_dict(case_id), ou.expected(case_id), kernel
    c = fu.bb144_case()
    return c, fu.expected("bb144", c, np.float32), kernel


@pytest.mark.parametrize("chunk,static_pct,want_llr", [(1, 0, True), (8, 50, True), (1, 50, True), (8, 0, True), (8, 50, False)],
                         ids=["chunk1-static0", "chunk8-static50", "chunk1-static50", "chunk8-static0", "chunk8-static50-nollr"])
@pytest.mark.parametrize("key", list(_POOL_CASES))
def test_work_pools(key, chunk, static_pct, want_llr):
    """20 011 rows drawn by index from a case's rows (rows are independent): static shares and pulls of 1 and 8 from the pooled counters,
    into poisoned outputs -- a row nobody decodes shows as missing, not as stale."""
    import torch
    c, want_rows, kernel = _pool_case(key)
    idx = (np.arange(POOL_ROWS, dtype=np.int64) * 37) % len(c["synd"])
    want = tuple(x[idx] for x in want_rows)
    assert not np.isnan(want[1]).any() and want[2].min() >= 1, "the poison must differ from every expected value"
    synd = torch.as_tensor(np.ascontiguousarray(c["synd"][idx]), device="cuda")
    eng = _engine(c, switches={"EDGE_CHUNK": chunk, "EDGE_STATIC_PCT": static_pct})
    try:
        out = _poisoned(POOL_ROWS, want[0].shape[1], want_llr)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(synd, want_llr=want_llr, out=out)
            torch.cuda.synchronize()
    finally:
        eng.close()
    assert all(g is o for g, o in zip(got, out))
    dec, llr, it, cv = (None if x is None else x.cpu().numpy() for x in got)
    if not want_llr:
        assert llr is None
        llr = want[1]
    assert set(np.unique(cv).tolist()) <= {0, 1}, "converge flags that were never written"
    _same((dec, llr, it, cv), want, f"{key} x {POOL_ROWS} rows, chunk {chunk}, static {static_pct} %")
    _assert_onchip(log, kernel)


# ---- 5. routing off ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["F32_ONCHIP=0", "small_mode=0", "F32_NT=0"])
@pytest.mark.parametrize("case_id", ["edge-R2-m17-percol", "edge8-DC4-R2-m4-uniform"])
def test_routing_off(case_id, how):
    mode, switches = {"F32_ONCHIP=0": (6, {"F32_ONCHIP": 0}), "small_mode=0": (0, {}), "F32_NT=0": (6, {"F32_NT": 0})}[how]
    got, log = _decode(ou.case_dict(case_id), mode, switches)
    _same(got, ou.expected(case_id), f"{case_id} with {how}")
    _assert_per_pass(log)


# ---- 6. dtype round trip on one engine ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["edge-R2-m17-percol", "edge8-DC3-R3-m17-percol"])
def test_dtype_round_trip(case_id, oracle_built):
    """float32, float64, float32, float64 on one handle: the slot tables are shared, the per-slot priors are written in the element type of
    the decode at hand -- neither dtype may read the other's."""
    case = next(c for c in ou.ONCHIP_CASES if c.id == case_id)
    assert not case.uniform
    c = ou.case_dict(case_id)
    eng = _engine(c, case.mode)
    try:
        for dtype in ("float32", "float64", "float32", "float64"):
            eng.set_message_dtype(dtype)
            with launch_util.launch_log() as log:
                got = eng.decode_batch(c["synd"])
            if dtype == "float32":
                _same(got, ou.expected(case_id), f"{case_id} in float32")
                _assert_onchip(log, ou.f32_kernel_name(case.kernel))
            else:
                want = lu.expected(case_id)
                for k, name in ((0, "decoding"), (2, "iterations"), (3, "converge")):
                    assert np.array_equal(got[k], np.asarray(want[k]).astype(got[k].dtype)), f"{case_id} in float64: {name}"
                assert bits_equal(got[1], np.asarray(want[1])), f"{case_id} in float64: log-ratios"
                assert launch_util.of(log, *lu.BP_DECODE_KERNELS) == [case.kernel] and log[case.kernel] == 1, sorted(log)
                launch_util.assert_not_ran(log, *ou.ONCHIP)
    finally:
        eng.close()


# ---- 7. around it --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["edge-R2-m17-percol", "edge8-DC3-R3-m17-uniform"])
def test_one_iteration(case_id):
    case = next(c for c in ou.ONCHIP_CASES if c.id == case_id)
    c = ou.case_dict(case_id, max_iter=1)
    want = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], 1, c["alpha"], np.float32)
    assert not want[3].all() and (want[2] == 1).all()
    got, log = _decode(c, case.mode)
    _same(got, want, f"{case_id}/max_iter=1")
    _assert_onchip(log, ou.f32_kernel_name(case.kernel))


@pytest.mark.parametrize("backend", ["cython", "ctypes"])
def test_single_decode(backend):
    """decode(): one row through the batch kernel."""
    c = fu.bb144_case()
    want = fu.expected("bb144", c, np.float32)
    d = _decoder(c, backend)
    for row in (int(np.flatnonzero(want[3] & c["synd"].any(axis=1))[0]), int(np.flatnonzero(~want[3])[0])):
        with launch_util.launch_log() as log:
            out = d.decode(c["synd"][row])
        _same((out[None, :], d.log_prob_ratios[None, :], np.array([d.iter]), np.array([d.converge])),
              tuple(x[row:row + 1] for x in want), f"bb144/decode row {row}/{backend}")
        _assert_onchip(log, "bp_edge8_f32_kernel<9, 3, true>")


@pytest.mark.parametrize("backend", ["cython", "ctypes"])
@pytest.mark.parametrize("key", ["bb144", "edge-R2-m17-percol"])
def test_decode_batch_host_arrays(key, backend):
    c, want = (fu.bb144_case(), None) if key == "bb144" else (ou.case_dict(key), ou.expected(key))
    want = want or fu.expected("bb144", c, np.float32)
    d = _decoder(c, backend)
    with launch_util.launch_log() as log:
        dec = d.decode_batch(c["synd"])
    _same((dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), _shortcut(want, c["synd"]), f"{key}/{backend}")
    assert d.log_prob_ratios_batch.dtype == np.float64 and d.log_prob_ratios_batch.shape == (len(c["synd"]), c["h"].shape[1])
    launch_util.assert_ran(log, "bp_edge8_f32_kernel<9, 3, true>" if key == "bb144" else "bp_edge_f32_kernel<2, false, false>")
    launch_util.assert_not_ran(log, *ou.PER_PASS)


@pytest.mark.parametrize("key", ["bb144", "edge-R2-m17-percol"])
def test_decode_batch_cuda_tensors(key):
    import torch
    c, want = (fu.bb144_case(), None) if key == "bb144" else (ou.case_dict(key), ou.expected(key))
    want = want or fu.expected("bb144", c, np.float32)
    d = _decoder(c)
    with launch_util.launch_log() as log:
        dec = d.decode_batch(torch.as_tensor(np.array(c["synd"]), device="cuda"))
        torch.cuda.synchronize()
    assert d.log_prob_ratios_batch.dtype == torch.float64
    _same((dec.cpu().numpy(), d.log_prob_ratios_batch.cpu().numpy(), d.iter_batch.cpu().numpy(), d.converge_batch.cpu().numpy()),
          _shortcut(want, c["synd"]), f"{key}/cuda")
    launch_util.assert_ran(log, "bp_edge8_f32_kernel<9, 3, true>" if key == "bb144" else "bp_edge_f32_kernel<2, false, false>")
    launch_util.assert_not_ran(log, *ou.PER_PASS)


@pytest.mark.parametrize("osd_method,osd_order,code", [("osd_0", 0, 1), ("osd_cs", 4, 3)])
def test_bposd(oracle_built, osd_method, osd_order, code):
    """BP + OSD on the widened float32 posteriors of the on-chip kernel (the expectation of tests/test_gpu_f32.py's BP + OSD test)."""
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    c = fu.bb144_case()
    dec32, llr32, it32, cv32 = fu.expected("bb144", c, np.float32)
    assert int((~cv32).sum()) >= 10
    orc = oracle_built.BpOracle(c["h"], error_channel=c["probs"], max_iter=c["max_iter"], bp_method="minimum_sum", ms_scaling_factor=c["alpha"])
    want = dec32.copy()
    for b in np.flatnonzero(~cv32):
        want[b] = orc.osdw(c["synd"][b], llr32[b], code, osd_order)[0]
    for backend in ("cython", "ctypes"):
        d = _decoder(c, backend, cls=BpOsdDecoder, osd_method=osd_method, osd_order=osd_order)
        with launch_util.launch_log() as log:
            got = d.decode_batch(c["synd"])
        _same((got, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), _shortcut((want, llr32, it32, cv32), c["synd"]), f"bb144/{osd_method}/{backend}")
        _assert_onchip(log, "bp_edge8_f32_kernel<9, 3, true>")
    row = int(np.flatnonzero(~cv32)[0])
    assert np.array_equal(d.decode(c["synd"][row]), want[row]), "BpOsdDecoder.decode in float32"


def test_close_frees_every_device_buffer():
    from ldpc_amd import _lib
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    for c in (fu.bb144_case(), ou.case_dict("edge-R2-m17-percol")):
        eng = _engine(c)
        try:
            eng.decode_batch(c["synd"])
            eng.set_message_dtype("float64")
            eng.decode_batch(c["synd"])
            eng.set_message_dtype("float32")
            eng.set_osd(1, 0)
            eng.decode_batch(c["synd"], osd=True)
            during = held()
        finally:
            eng.close()
        after = held()
        print(f"float32 on chip: device buffer bytes before {before}, with the engine {during}, after close {after}")
        assert during > before and after == before, f"{after - before} bytes of device buffers outlive the handle"


# ---- 8. refusals stand -------------------------------------------------------------------------------------------------------------------
def test_refusals_stand_on_a_code_the_route_takes():
    from ldpc_amd import _lib
    c = fu.small_case("hamming3", 0.625)  # (test_special_values: bp_edge8_f32_kernel<2, 3, false>)
    eng = _engine(c, method=0)  # product-sum
    try:
        _refusals_then_a_decode(eng, c)
    finally:
        eng.close()


def _refusals_then_a_decode(eng, c):
    from ldpc_amd import _lib
    with pytest.raises(_lib.LdpcHipError, match=r"error -4: float32 messages: product-sum"):
        eng.decode_batch(c["synd"])
    eng.set_params(c["max_iter"], 1, 0.625)
    eng.set_schedule("serial")
    with pytest.raises(_lib.LdpcHipError, match=r"error -4: float32 messages: the serial schedules"):
        eng.decode_batch(c["synd"])
    eng.set_schedule("parallel")
    for osd0 in (False, True):
        with pytest.raises(_lib.LdpcHipError, match=r"error -4: float32 messages: per-row channel probabilities"):
            eng.decode_batch(c["synd"], osd0=osd0, channel_probs=np.tile(c["probs"], (len(c["synd"]), 1)))
    with pytest.raises(_lib.LdpcHipError, match=r"error -4: float32 messages: soft-syndrome"):
        eng.soft_info_decode_batch(np.ones((2, 3)), np.inf, 2.0)
    with launch_util.launch_log() as log:  # ... and the handle still decodes, on chip
        got = eng.decode_batch(c["synd"])
    _same(got, fu.expected("hamming3_a0.625", c, np.float32), "hamming3 after the refusals")
    _assert_onchip(log, "bp_edge8_f32_kernel<2, 3, false>")
