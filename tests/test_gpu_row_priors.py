"""``decode_batch(..., channel_probs=P)`` on the GPU: every row decoded with its own channel probabilities, compared BIT FOR BIT -- decisions,
converge flags, iteration counts, log-ratio bit patterns (``oracle.bits_equal``) -- with what the reference's own
``update_channel_probs(P[b]); decode(S[b])`` loop returned (tests/golden/row_priors/), through the Python API (host arrays, device
tensors, both bindings), the C ABI (sync, async), every forced kernel path, and against the real reference compiled under oracle/_ref."""
import numpy as np
import pytest

import launch_util
import oracle
from row_priors_util import case_names, llr_digest, load_case, ran_bp

pytestmark = pytest.mark.gpu

CASES = case_names()
_LOADED: dict = {}


def _case(name):
    if name not in _LOADED:
        c = load_case(name)
        for k in ("probs", "syndromes", "decoding", "converge", "iterations", "llr", "llr_crc"):
            c[k].setflags(write=False)
        _LOADED[name] = c
    return _LOADED[name]


def _engine(c):
    from ldpc_amd.engine import HipBpEngine
    h = c["h"]
    return HipBpEngine(h.indptr, h.indices, c["n"], np.full(c["n"], c["own_p"]), c["max_iter"], 0 if c["bp_method"] == "product_sum" else 1,
                       c["ms_scaling_factor"])


def _decoder(c, **kw):
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    args = dict(error_rate=c["own_p"], max_iter=c["max_iter"], bp_method=c["bp_method"], ms_scaling_factor=c["ms_scaling_factor"], **kw)
    return BpOsdDecoder(c["h"], osd_method="osd_0", **args) if c["osd"] else BpDecoder(c["h"], input_vector_type="syndrome", **args)


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same_as_fixture(c, dec, llr, it, cv, rows=None):
    """``rows``: the rows to compare (the C ABI runs BP on an all-zero syndrome too; the Python layer applies the reference's shortcut)."""
    rows = np.ones(len(dec), bool) if rows is None else rows
    dec, llr, it, cv = _np(dec), _np(llr), _np(it), _np(cv).astype(bool)
    print(f"{c['name']}: decisions differ in {int((dec[rows] != c['decoding'][rows]).any(axis=1).sum())} rows, flags in {int((cv[rows] != c['converge'][rows]).sum())}, "
          f"iterations in {int((it[rows] != c['iterations'][rows]).sum())}, log-ratio checksums in {int((llr_digest(llr)[rows] != c['llr_crc'][rows]).sum())} of {int(rows.sum())}")
    assert np.array_equal(dec[rows], c["decoding"][rows]), "hard decisions differ from the reference's loop"
    assert np.array_equal(cv[rows], c["converge"][rows]), "converge flags differ"
    assert np.array_equal(it[rows], c["iterations"][rows]), "iteration counts differ"
    k = np.flatnonzero(rows[:len(c["llr"])])
    assert oracle.bits_equal(llr[k], c["llr"][k]), "log-ratios (rows stored in full) are not the reference's bits"
    assert np.array_equal(llr_digest(llr)[rows], c["llr_crc"][rows]), "log-ratio bit patterns differ in some row"


@pytest.mark.parametrize("backend", ["default", "ctypes"])
@pytest.mark.parametrize("name", CASES)
def test_python_api_host_arrays(name, backend):
    c = _case(name)
    d = _decoder(c, **({} if backend == "default" else {"_backend": "ctypes"}))
    dec = d.decode_batch(c["syndromes"], channel_probs=c["probs"])
    _same_as_fixture(c, dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch)
    assert np.array_equal(d.channel_probs, np.full(c["n"], c["own_p"])), "the decoder's own probabilities must stay"


@pytest.mark.parametrize("name", CASES)
def test_python_api_device_tensors(name):
    import torch
    c = _case(name)
    d = _decoder(c)
    s, p = torch.from_numpy(c["syndromes"].copy()).cuda(), torch.from_numpy(c["probs"].copy()).cuda()
    dec = d.decode_batch(s, channel_probs=p)
    assert dec.is_cuda and d.log_prob_ratios_batch.is_cuda
    _same_as_fixture(c, dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch)
    with pytest.raises(ValueError, match="same place as the syndromes"):
        d.decode_batch(s, channel_probs=c["probs"])


@pytest.mark.parametrize("mode", ["host_sync", "device_sync", "device_async"])
@pytest.mark.parametrize("name", CASES)
def test_c_abi(name, mode):
    """ldpc_hip_bp_decode_batch_priors / ldpc_hip_bposd0_decode_batch_priors and their _async forms (the engine is their ctypes binding)."""
    import torch
    c = _case(name)
    eng = _engine(c)
    try:
        if mode == "host_sync":
            out = eng.decode_batch(c["syndromes"], osd0=c["osd"], channel_probs=c["probs"])
        else:
            s, p = torch.from_numpy(c["syndromes"].copy()).cuda(), torch.from_numpy(c["probs"].copy()).cuda()
            out = eng.decode_batch(s, osd0=c["osd"], channel_probs=p, asynchronous=mode == "device_async")
            torch.cuda.synchronize()
        _same_as_fixture(c, *out, rows=ran_bp(c))
    finally:
        eng.close()


@pytest.mark.skipif(not oracle.have_ref(), reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("name", CASES)
def test_against_the_compiled_reference(name):
    """The same inputs through the real reference (oracle/_ref): ``set_channel(P[b])`` then a one-row decode, every log-ratio in full."""
    c = _case(name)
    eng = _engine(c)
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
        assert oracle.bits_equal(llr[b], rl[0]), f"row {b}: log-ratios"


def _raw(eng, c, **kw):
    return [_np(x) for x in eng.decode_batch(c["syndromes"], osd0=c["osd"], **kw)]


def _assert_same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and oracle.bits_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["row_priors_irregular_n600_ps16", "row_priors_irregular_n600_ms16_adaptive"])
def test_chunked_priors(name):
    """max_chunk_tiles = 1: three chunks, chunk c must read rows [64 c, ...) of the probabilities."""
    c = _case(name)
    eng = _engine(c)
    try:
        eng.set_tuning(max_chunk_tiles=1)
        _same_as_fixture(c, *eng.decode_batch(c["syndromes"], channel_probs=c["probs"]), rows=ran_bp(c))
    finally:
        eng.close()


@pytest.mark.parametrize("small_mode", [0, 2])
@pytest.mark.parametrize("name", ["row_priors_hamming3_ps", "row_priors_hamming3_ms", "row_priors_bb144_ps10_osd0"])
def test_forced_kernel_family(name, small_mode):
    """set_small_code_kernel(0): a small code on the per-pass kernels; (2): the slot kernel."""
    c = _case(name)
    eng = _engine(c)
    try:
        eng.set_small_code_kernel(small_mode)
        with launch_util.launch_log() as log:
            out = eng.decode_batch(c["syndromes"], osd0=c["osd"], channel_probs=c["probs"])
        _same_as_fixture(c, *out, rows=ran_bp(c))
        # the forced family ran, in its row-prior form (RP, the last template argument) and in no other
        family = ("bp_spread_init_kernel", "bp_spread_bit_kernel", "bp_spread_finish_kernel") if small_mode == 0 else ("bp_small_kernel",)
        for kernel in family:
            ran = launch_util.of(log, kernel)
            assert ran and all(k.endswith(", true>") for k in ran), (kernel, sorted(log))
        others = {"bp_small_kernel", "bp_wave_kernel", "bp_wave_ps_kernel", "bp_edge_kernel", "bp_edge8_kernel", "bp_decode_kernel", "bp_spread_init_kernel"} - set(family)
        launch_util.assert_not_ran(log, *sorted(others))
    finally:
        eng.close()


@pytest.mark.parametrize("small_mode", [-1, 0, 2])
@pytest.mark.parametrize("name", ["row_priors_hamming3_ps", "row_priors_irregular_n600_ms16_a0625", "row_priors_bb144_ps10_osd0"])
def test_own_priors_in_every_row_equal_the_plain_decode_and_leave_the_handle_alone(name, small_mode):
    """Rows of the handle's own probabilities give the plain decode's bits; a plain decode after a row-prior call gives the same bits as before it."""
    c = _case(name)
    eng = _engine(c)
    try:
        eng.set_small_code_kernel(small_mode)
        before = _raw(eng, c)
        _assert_same(_raw(eng, c, channel_probs=np.full(c["probs"].shape, c["own_p"])), before)
        eng.decode_batch(c["syndromes"], osd0=c["osd"], channel_probs=c["probs"])
        _assert_same(_raw(eng, c), before)
    finally:
        eng.close()


def test_one_iteration_and_a_single_row():
    """max_iter = 1 (the per-pass path's only round is also its last) and B = 1, against the CPU restatement."""
    c = _case("row_priors_irregular_n600_ps16")
    from ldpc_amd.engine import HipBpEngine
    h = c["h"]
    eng = HipBpEngine(h.indptr, h.indices, c["n"], np.full(c["n"], c["own_p"]), 1, 0, 1.0)
    try:
        for rows in (slice(0, 70), slice(3, 4)):
            s, p = c["syndromes"][rows], c["probs"][rows]
            dec, llr, it, cv = eng.decode_batch(s, channel_probs=p)
            for b in range(len(s)):
                od, ol, oi, oc = oracle.BpOracle(h, error_channel=p[b], max_iter=1, bp_method="product_sum").decode_batch(s[b:b + 1])
                assert np.array_equal(dec[b], od[0]) and int(it[b]) == int(oi[0]) and bool(cv[b]) == bool(oc[0]) and oracle.bits_equal(llr[b], ol[0]), f"row {b}"
    finally:
        eng.close()


def test_c_abi_refuses_serial_schedules_and_bad_host_probabilities():
    from ldpc_amd import _lib
    c = _case("row_priors_hamming3_ms")
    eng = _engine(c)
    try:
        eng.set_schedule("serial")
        with pytest.raises(_lib.LdpcHipError, match="error -4.*serial schedules"):
            eng.decode_batch(c["syndromes"], channel_probs=c["probs"])
        eng.set_schedule("parallel")
        lib, s, p = _lib.load(), c["syndromes"], c["probs"].copy()
        p[2, 1] = 1.25  # (past the Python layer's own check: straight into the C entry point)
        dec, it, cv = np.zeros((70, 7), np.uint8), np.zeros(70, np.int32), np.zeros(70, np.uint8)
        rc = lib.ldpc_hip_bp_decode_batch_priors(eng._h, s.ctypes.data, 70, dec.ctypes.data, None, it.ctypes.data, cv.ctypes.data, p.ctypes.data)
        assert rc == -1 and b"channel_probs[2][1]" in lib.ldpc_hip_last_error()
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["row_priors_irregular_n600_ps16", "row_priors_hamming3_ps", "row_priors_bb144_ps10_osd0"])
def test_close_frees_every_device_buffer(name):
    """tests/test_gpu_buffer_leak.py's method on a handle that ran a row-prior decode (its priors buffer and staging are DeviceBufs)."""
    from ldpc_amd import _lib
    c = _case(name)
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    eng = _engine(c)
    eng.decode_batch(c["syndromes"], osd0=c["osd"], channel_probs=c["probs"])
    during = held()
    eng.close()
    after = held()
    print(f"{name}: device buffer bytes before {before}, with the engine {during}, after close {after}")
    assert during >= before + c["probs"].nbytes, "the decode went through no counted priors buffer"
    assert after == before, f"{after - before} bytes of device buffers outlive the handle"
