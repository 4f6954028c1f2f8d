"""``decode_batch(..., channel_probs=P)`` on the codes of the lane = edge families: bp_edge_rp_kernel<R> and bp_edge8_rp_kernel<R, DC>
(ldpc_amd/csrc/bp_edge_rp_kernel.h) against the per-row oracle and the reference's own fixtures -- hard decisions, converge flags, iteration
counts and the bit patterns of the log-ratios -- on a smallest code for every instantiation (tests/row_priors_edge_util.py;
tests/test_row_priors_edge_cases.py checks the cases without a GPU), with the launch log showing that exactly the named instantiation ran.
Then what is new about the route: a wavefront must read the priors of the row it PULLED (work pools, 20 011 rows), the routing (EDGE_RP,
forced kernel families, product-sum, codes no edge plan takes), a handle that goes from plain to row-prior decodes and back, device
tensors and the _async entry point, and that close() frees every buffer.  EDGE_RP = 1 is set wherever a kernel is named, except in the
test of the default."""
import numpy as np
import pytest
import scipy.sparse as sp

import ladder_util as lu
import launch_util
import row_priors_edge_util as ru
import oracle
from oracle import bits_equal
from row_priors_util import llr_digest, ran_bp

pytestmark = pytest.mark.gpu

OTHER_BP = tuple(k for k in lu.BP_DECODE_KERNELS)  # every plain BP decode kernel: a row-prior edge decode launches none of them


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


def _same(got, want, what):
    dec, llr, it, cv = (_np(x) for x in got)
    print(f"{what}: {int((dec != want[0]).any(axis=1).sum())} rows differ in decisions, {int(np.count_nonzero(cv.astype(bool) != want[3]))} in flags, "
          f"{int(np.count_nonzero(it != want[2]))} in iteration counts, {int(np.count_nonzero(llr_digest(llr) != llr_digest(want[1])))} in log-ratio bits, of {len(dec)}")
    assert np.array_equal(dec, want[0]), f"{what}: hard decisions"
    assert np.array_equal(cv.astype(bool), want[3]), f"{what}: converge flags"
    assert np.array_equal(it, want[2]), f"{what}: iteration counts"
    assert bits_equal(llr, want[1]), f"{what}: log-ratios differ in some bit"


def _assert_rp(log, name):
    """Exactly the named row-prior instantiation, once; no other BP decode kernel."""
    launch_util.assert_resolved(log)
    assert launch_util.of(log, *ru.RP_KERNELS) == [name], f"expected exactly {name}; the log has {sorted(log)}"
    assert log[name] == 1
    launch_util.assert_not_ran(log, *OTHER_BP)
    launch_util.assert_ran(log, "row_priors_rowmajor_kernel")


def _assert_no_rp(log):
    launch_util.assert_not_ran(log, *ru.RP_KERNELS, "row_priors_rowmajor_kernel")


def _ladder_decode(case_id, mode, switches, method=None, special=True, **kw):
    c = next(c for c in lu.ALL_CASES if c.id == case_id)
    h, own, synd = lu.inputs(case_id)
    eng = _engine(h, own, lu.MAX_ITER, c.alpha, method or c.method, mode, switches)
    try:
        with launch_util.launch_log() as log:
            out = eng.decode_batch(synd, channel_probs=ru.row_probs(case_id, special), **kw)
    finally:
        eng.close()
    return out, log


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ru.CASES, ids=[c.id for c in ru.CASES])
def test_every_instantiation(case):
    got, log = _ladder_decode(case.id, case.mode, {**case.switches, "EDGE_RP": 1})
    _same(got, ru.expected(case.id), case.id)
    _assert_rp(log, ru.rp_kernel_name(case.kernel))


# ---- 2. the reference's fixtures -----------------------------------------------------------------------------------------------------------
_FIXTURE_KERNEL = {"row_priors_rep5_ms": "bp_edge_rp_kernel<1>", "row_priors_hamming3_ms": "bp_edge8_rp_kernel<2, 3>",
                   "row_priors_bb144_ms10_osd0": "bp_edge8_rp_kernel<9, 3>", "row_priors_surface_ms_adaptive": "bp_edge_rp_kernel<1>"}


@pytest.mark.parametrize("name", list(_FIXTURE_KERNEL))
def test_fixtures(name):
    """The reference's ``update_channel_probs(P[b]); decode(S[b])`` loop; the BB144 fixture through ldpc_hip_bposd0_decode_batch_priors."""
    c = ru.load_fixture(name)
    eng = _engine(c["h"], np.full(c["n"], c["own_p"]), c["max_iter"], c["ms_scaling_factor"], c["bp_method"], switches={"EDGE_RP": 1})
    try:
        with launch_util.launch_log() as log:
            out = eng.decode_batch(c["syndromes"], osd0=c["osd"], channel_probs=c["probs"])
    finally:
        eng.close()
    assert c["osd"] == (name == "row_priors_bb144_ms10_osd0")
    _same_as_fixture(c, *out, rows=ran_bp(c))  # (the C ABI runs BP on an all-zero syndrome too; the fixture holds the reference's shortcut for it)
    _assert_rp(log, _FIXTURE_KERNEL[name])


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


# The two new fixtures through the other entry points (those of tests/golden/row_priors/ go through them in tests/test_gpu_row_priors.py):
# the Python classes with host arrays under both bindings and with device tensors, the _async C entry point, the compiled reference.
def _decoder(c, **kw):
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    args = dict(error_rate=c["own_p"], max_iter=c["max_iter"], bp_method=c["bp_method"], ms_scaling_factor=c["ms_scaling_factor"], **kw)
    return BpOsdDecoder(c["h"], osd_method="osd_0", **args) if c["osd"] else BpDecoder(c["h"], input_vector_type="syndrome", **args)


@pytest.mark.parametrize("how", ["default", "ctypes", "device_tensors"])
@pytest.mark.parametrize("name", ru.EDGE_FIXTURES)
def test_new_fixtures_python_api(name, how):
    import torch
    c = ru.load_fixture(name)
    d = _decoder(c, **({"_backend": "ctypes"} if how == "ctypes" else {}))
    s, p = c["syndromes"], c["probs"]
    if how == "device_tensors":
        s, p = torch.from_numpy(s.copy()).cuda(), torch.from_numpy(p.copy()).cuda()
    dec = d.decode_batch(s, channel_probs=p)
    _same_as_fixture(c, dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch)
    assert np.array_equal(d.channel_probs, np.full(c["n"], c["own_p"])), "the decoder's own probabilities must stay"


@pytest.mark.parametrize("name", ru.EDGE_FIXTURES)
def test_new_fixtures_async_c_abi(name):
    import torch
    c = ru.load_fixture(name)
    eng = _engine(c["h"], np.full(c["n"], c["own_p"]), c["max_iter"], c["ms_scaling_factor"], c["bp_method"], switches={"EDGE_RP": 1})
    try:
        s, p = torch.from_numpy(c["syndromes"].copy()).cuda(), torch.from_numpy(c["probs"].copy()).cuda()
        with launch_util.launch_log() as log:
            out = eng.decode_batch(s, osd0=c["osd"], channel_probs=p, asynchronous=True)
            torch.cuda.synchronize()
        _same_as_fixture(c, *out, rows=ran_bp(c))
        _assert_rp(log, _FIXTURE_KERNEL[name])
    finally:
        eng.close()


@pytest.mark.skipif(not oracle.have_ref(), reason="oracle/_ref not built (needs the reference's sources)")
@pytest.mark.parametrize("name", ru.EDGE_FIXTURES)
def test_new_fixtures_against_the_compiled_reference(name):
    """The same inputs through the real reference where it is built: ``set_channel(P[b])`` then a one-row decode, every log-ratio in full."""
    c = ru.load_fixture(name)
    eng = _engine(c["h"], np.full(c["n"], c["own_p"]), c["max_iter"], c["ms_scaling_factor"], c["bp_method"], switches={"EDGE_RP": 1})
    try:
        dec, llr, it, cv = eng.decode_batch(c["syndromes"], osd0=c["osd"], channel_probs=c["probs"])
    finally:
        eng.close()
    kw = dict(max_iter=c["max_iter"], bp_method=c["bp_method"], ms_scaling_factor=c["ms_scaling_factor"])
    ref = None if c["osd"] else oracle.RefBp(c["h"], error_rate=c["own_p"], **kw)
    for b in np.flatnonzero(ran_bp(c)):
        if c["osd"]:
            rd, rl, ri, rc = oracle.RefBpOsd(c["h"], error_channel=c["probs"][b], **kw).decode_batch(c["syndromes"][b:b + 1])
        else:
            ref.set_channel(c["probs"][b])
            rd, rl, ri, rc = ref.decode_batch(c["syndromes"][b:b + 1])
        assert np.array_equal(dec[b], rd[0]) and bool(cv[b]) == bool(rc[0]) and int(it[b]) == int(ri[0]), f"row {b}"
        assert bits_equal(llr[b], rl[0]), f"row {b}: log-ratios"


# ---- 3. work pools: a wavefront reads the priors of the row it pulled ------------------------------------------------------------------
def _poisoned(b, n, want_llr=True):
    """Output tensors no decode leaves as they are: 0xFF bytes (decisions and flags are 0 / 1, iteration counts positive), NaN."""
    import torch
    return (torch.full((b, n), 0xFF, dtype=torch.uint8, device="cuda"),
            torch.full((b, n), float("nan"), dtype=torch.float64, device="cuda") if want_llr else None,
            torch.full((b,), -1, dtype=torch.int32, device="cuda"), torch.full((b,), 0xFF, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("chunk,static_pct,want_llr", [(1, 0, True), (8, 50, True), (1, 50, True), (8, 0, True), (8, 50, False)],
                         ids=["chunk1-static0", "chunk8-static50", "chunk1-static50", "chunk8-static0", "chunk8-static50-nollr"])
@pytest.mark.parametrize("key", list(ru.POOL_CASES))
def test_work_pools(key, chunk, static_pct, want_llr):
    """20 011 rows drawn by index -- syndromes AND priors with the same index -- from a case's rows: static shares and pulls of 1 and 8
    from the pooled counters, into poisoned outputs.  Neighbouring rows of the batch are 37 rows apart in the case, with different priors:
    a wavefront that kept its previous row's priors, or took those of its own index, decodes to other bits."""
    import torch
    h, own, synd_rows, probs_rows, max_iter, alpha, want_rows, kernel = ru.pool_inputs(key)
    idx = ru.pool_index(len(synd_rows))
    want = tuple(x[idx] for x in want_rows)
    assert not np.isnan(want[1]).any() and want[2].min() >= 1, "the poison must differ from every expected value"
    synd = torch.as_tensor(np.ascontiguousarray(synd_rows[idx]), device="cuda")
    probs = torch.as_tensor(np.ascontiguousarray(probs_rows[idx]), device="cuda")
    eng = _engine(h, own, max_iter, alpha, mode=6, switches={"EDGE_RP": 1, "EDGE_CHUNK": chunk, "EDGE_STATIC_PCT": static_pct})
    try:
        out = _poisoned(ru.POOL_ROWS, h.shape[1], want_llr)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(synd, want_llr=want_llr, out=out, channel_probs=probs)
            torch.cuda.synchronize()
    finally:
        eng.close()
    assert all(g is o for g, o in zip(got, out))
    dec, llr, it, cv = (_np(x) for x in got)
    if not want_llr:
        assert llr is None
        llr = want[1]
    assert set(np.unique(cv).tolist()) <= {0, 1}, "converge flags that were never written"
    _same((dec, llr, it, cv), want, f"{key} x {ru.POOL_ROWS} rows, chunk {chunk}, static {static_pct} %")
    _assert_rp(log, kernel)


# ---- 4. routing ------------------------------------------------------------------------------------------------------------------------------
_ROUTE_CASES = ["edge-R2-m17-percol", "edge8-DC3-R3-m17-percol"]


@pytest.mark.parametrize("how", ["EDGE_RP=0", "small_mode=2", "small_mode=0"])
@pytest.mark.parametrize("case_id", _ROUTE_CASES)
def test_routing_off(case_id, how):
    """EDGE_RP = 0 and mode 2: the slot kernel in its row-prior form; mode 0: the per-pass kernels -- today's kernels, the same bits."""
    mode, switches = {"EDGE_RP=0": (6, {"EDGE_RP": 0}), "small_mode=2": (2, {"EDGE_RP": 1}), "small_mode=0": (0, {"EDGE_RP": 1})}[how]
    got, log = _ladder_decode(case_id, mode, switches)
    _same(got, ru.expected(case_id), f"{case_id} with {how}")
    _assert_no_rp(log)
    family = ("bp_spread_init_kernel", "bp_spread_bit_kernel", "bp_spread_finish_kernel") if mode == 0 else ("bp_small_kernel",)
    for kernel in family:
        ran = launch_util.of(log, kernel)
        assert ran and all(k.endswith(", true>") for k in ran), (kernel, sorted(log))
    launch_util.assert_not_ran(log, *({"bp_small_kernel", "bp_edge_kernel", "bp_edge8_kernel", "bp_wave_kernel", "bp_spread_init_kernel"} - set(family)))


@pytest.mark.parametrize("mode", [-1, 1, 6])
@pytest.mark.parametrize("case_id", _ROUTE_CASES)
def test_default_route(case_id, mode):
    """EDGE_RP unset: the route is the default in modes -1, 1 and 6 (the measurement's rule: DESIGN.md section 4, NOTES.md)."""
    c = next(c for c in lu.ALL_CASES if c.id == case_id)
    got, log = _ladder_decode(case_id, mode, {})
    _same(got, ru.expected(case_id), f"{case_id}, mode {mode}, EDGE_RP unset")
    _assert_rp(log, ru.rp_kernel_name(c.kernel))


@pytest.mark.parametrize("case_id", _ROUTE_CASES)
def test_product_sum_never_takes_the_route(case_id):
    got, log = _ladder_decode(case_id, 6, {"EDGE_RP": 1}, method="product_sum")
    _same(got, ru.expected(case_id, method="product_sum"), f"{case_id}, product-sum")
    _assert_no_rp(log)


_OUTSIDE = [c for c in lu.OUTSIDE_CASES if c.kernel is None]


@pytest.mark.parametrize("case", _OUTSIDE, ids=[c.id for c in _OUTSIDE])
def test_codes_no_edge_plan_takes(case):
    got, log = _ladder_decode(case.id, case.mode, {"EDGE_RP": 1})
    _same(got, ru.expected(case.id), case.id)
    _assert_no_rp(log)


# ---- 5. the handle is left alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["edge-R2-m17-percol", "edge8-DC3-R3-m17-percol", "edge-R2-m17-noclamp", "edge8-DC4-R2-m4-uniform"])
def test_plain_decodes_around_a_row_prior_decode(case_id):
    """plain, row priors, plain on one handle: the plain decodes are bit-identical, still launch the plain kernel (whose per-slot priors the
    row-prior kernels never touch), and rows of the handle's own probabilities give the plain decode's bits -- with a uniform handle that
    sets the clamped row-prior form against bp_edge_kernel's NOCLAMP form."""
    c = next(c for c in lu.ALL_CASES if c.id == case_id)
    h, own, synd = lu.inputs(case_id)
    rp_name = ru.rp_kernel_name(c.kernel.replace("true", "false"))
    eng = _engine(h, own, lu.MAX_ITER, c.alpha, mode=c.mode, switches={**c.switches, "EDGE_RP": 1})
    try:
        with launch_util.launch_log() as log:
            before = eng.decode_batch(synd)
        assert launch_util.of(log, *lu.BP_DECODE_KERNELS) == [c.kernel], sorted(log)
        _same(before, lu.expected(case_id), f"{case_id}: plain decode")
        with launch_util.launch_log() as log:
            own_rows = eng.decode_batch(synd, channel_probs=np.tile(own, (len(synd), 1)))
        _assert_rp(log, rp_name)
        _same(own_rows, before, f"{case_id}: rows of the handle's own probabilities")
        with launch_util.launch_log() as log:
            got = eng.decode_batch(synd, channel_probs=ru.row_probs(case_id))
        _assert_rp(log, rp_name)
        if not c.uniform:
            _same(got, ru.expected(case_id), f"{case_id}: row priors")
        with launch_util.launch_log() as log:
            after = eng.decode_batch(synd)
        assert launch_util.of(log, *lu.BP_DECODE_KERNELS) == [c.kernel], sorted(log)
        _assert_no_rp(log)
        _same(after, before, f"{case_id}: plain decode after the row-prior decodes")
    finally:
        eng.close()


# ---- 6. device tensors and the _async entry point -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("asynchronous", [False, True], ids=["sync", "async"])
def test_device_tensors(asynchronous):
    import torch
    case_id = "edge8-DC3-R3-m17-percol"
    _, _, synd = lu.inputs(case_id)
    s, p = torch.from_numpy(np.array(synd)).cuda(), torch.from_numpy(np.array(ru.row_probs(case_id))).cuda()
    c = next(c for c in lu.ALL_CASES if c.id == case_id)
    h, own, _ = lu.inputs(case_id)
    eng = _engine(h, own, lu.MAX_ITER, c.alpha, mode=c.mode, switches={"EDGE_RP": 1})
    try:
        with launch_util.launch_log() as log:
            got = eng.decode_batch(s, channel_probs=p, asynchronous=asynchronous)
            torch.cuda.synchronize()
        assert all(x.is_cuda for x in got)
        _same(got, ru.expected(case_id), f"{case_id}, device tensors, {'async' if asynchronous else 'sync'}")
        _assert_rp(log, "bp_edge8_rp_kernel<3, 3>")
    finally:
        eng.close()


# ---- 7. close() ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["edge-R2-m17-percol", "edge8-DC3-R3-m17-percol"])
def test_close_frees_every_device_buffer(case_id):
    from ldpc_amd import _lib
    c = next(c for c in lu.ALL_CASES if c.id == case_id)
    h, own, synd = lu.inputs(case_id)
    probs = ru.row_probs(case_id)
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    eng = _engine(h, own, lu.MAX_ITER, c.alpha, mode=c.mode, switches={"EDGE_RP": 1})
    try:
        with launch_util.launch_log() as log:
            eng.decode_batch(synd, channel_probs=probs)
        during = held()
    finally:
        eng.close()
    after = held()
    _assert_rp(log, ru.rp_kernel_name(c.kernel))
    print(f"{case_id}: device buffer bytes before {before}, with the engine {during}, after close {after}")
    assert during >= before + probs.nbytes, "the decode went through no counted buffer for the rows' log-ratios"
    assert after == before, f"{after - before} bytes of device buffers outlive the handle"
