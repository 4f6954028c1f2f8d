"""The float32 message mode on the device against its NumPy restatement (tests/f32_util.py; tests/test_f32_restatement.py pins that
restatement's operation order to the oracle at float64): hard decisions, converge flags, iteration counts and the bit patterns of the
log-ratios, through BpDecoder.decode_batch on host arrays with both backends, CUDA tensors, the engine's synchronous and asynchronous
entry points, chunked batches, BP + OSD, and back to float64 on the same decoder.  Plus what the C ABI refuses, and that close() frees
every buffer the mode grew.

From test_tile_list_loops_and_compaction on: what only large batches reach -- the looping form of the per-round kernels (workgroup rows
that serve several slots of the tile list: switch F32_GRID_ROWS), bp_f32_compact_kernel beyond its first 64 entries, tiles that are
final but still listed, 4 and 16 nodes per wavefront, and the host's look at the flag that stops the queueing of rounds -- on batches of
70 tiles whose tiles end at chosen iterations (f32_util.scheduled_batch; tests/test_f32_restatement.py pins the schedule's properties).
Every output buffer is poisoned first, so a tile that is dropped shows as missing outputs, not as stale equal ones."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import f32_util as fu
import launch_util
from golden_util import load_case
from oracle import bits_equal

pytestmark = pytest.mark.gpu

CASES = {f"{code}_a{alpha}": (lambda code=code, alpha=alpha: fu.small_case(code, alpha))
         for code in ("hamming3", "rep5") for alpha in (0.625, 1.0, 0.0)}
CASES.update(degree1_empty=fu.degree1_case, irregular600=fu.irregular_case, heavy_rows=fu.heavy_rows_case)


def _same(got, want, what):
    dec, llr, it, cv = got
    print(f"{what}: {int(np.count_nonzero(np.asarray(dec) != want[0]))} decisions, {int(np.count_nonzero(np.asarray(cv, bool) != want[3]))} flags, "
          f"{int(np.count_nonzero(np.asarray(it) != want[2]))} iteration counts differ")
    assert np.array_equal(np.asarray(dec), want[0]), f"{what}: hard decisions"
    assert np.array_equal(np.asarray(cv, bool), want[3]), f"{what}: converge flags"
    assert np.array_equal(np.asarray(it), want[2]), f"{what}: iteration counts"
    assert bits_equal(np.asarray(llr), want[1]), f"{what}: log-ratios differ in some bit"


def _shortcut(want, synd):
    """What BpDecoder.decode_batch reports: all-zero rows take the host shortcut (zeros, converged, 0 iterations)."""
    dec, llr, it, cv = (x.copy() for x in want)
    zero = ~synd.any(axis=1)
    dec[zero], llr[zero], it[zero], cv[zero] = 0, 0.0, 0, True
    return dec, llr, it, cv


def _decoder(c, backend=None, cls=None, **kw):
    from ldpc_amd.bp_decoder import BpDecoder
    d = (cls or BpDecoder)(c["h"], error_channel=list(c["probs"]), max_iter=c["max_iter"], bp_method="minimum_sum",
                           ms_scaling_factor=c["alpha"], input_vector_type="syndrome", **({"_backend": backend} if backend else {}), **kw)
    d.message_dtype = "float32"
    return d


def _engine(c, method=1):
    from ldpc_amd.engine import HipBpEngine
    h = c["h"]
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], c["probs"], c["max_iter"], method, c["alpha"])
    eng.set_message_dtype("float32")
    return eng


@pytest.mark.parametrize("backend", ["cython", "ctypes"])
@pytest.mark.parametrize("key", list(CASES))
def test_decode_batch_host_arrays(key, backend):
    c = CASES[key]()
    d = _decoder(c, backend)
    dec = d.decode_batch(c["synd"])
    _same((dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), _shortcut(fu.expected(key, c, np.float32), c["synd"]), f"{key}/{backend}")
    assert d.log_prob_ratios_batch.dtype == np.float64 and d.log_prob_ratios_batch.shape == (len(c["synd"]), c["h"].shape[1])


@pytest.mark.parametrize("key", list(CASES))
def test_decode_batch_cuda_tensors(key):
    import torch
    c = CASES[key]()
    d = _decoder(c)
    dec = d.decode_batch(torch.as_tensor(c["synd"], device="cuda"))
    assert d.log_prob_ratios_batch.dtype == torch.float64
    _same((dec.cpu().numpy(), d.log_prob_ratios_batch.cpu().numpy(), d.iter_batch.cpu().numpy(), d.converge_batch.cpu().numpy()),
          _shortcut(fu.expected(key, c, np.float32), c["synd"]), f"{key}/cuda")


@pytest.mark.parametrize("key", list(CASES))
def test_engine_sync_and_async(key):
    import torch
    c = CASES[key]()
    want = fu.expected(key, c, np.float32)
    eng = _engine(c)
    assert eng.message_dtype() == "float32"
    _same(eng.decode_batch(c["synd"]), want, f"{key}/engine host")
    s = torch.as_tensor(c["synd"], device="cuda")
    for asynchronous in (False, True):
        out = eng.decode_batch(s, asynchronous=asynchronous)
        torch.cuda.current_stream().synchronize()
        _same(tuple(x.cpu().numpy() for x in out), want, f"{key}/engine device, asynchronous={asynchronous}")
    dec, llr, it, cv = eng.decode_batch(c["synd"], want_llr=False)
    assert llr is None and np.array_equal(dec, want[0]) and np.array_equal(it, want[2])
    eng.close()


def test_irregular_in_chunks_of_one_tile():
    c = fu.irregular_case()
    eng = _engine(c)
    eng.set_tuning(max_chunk_tiles=1)  # 130 rows: three chunks, the last of two rows
    _same(eng.decode_batch(c["synd"]), fu.expected("irregular600", c, np.float32), "irregular600/max_chunk_tiles=1")
    eng.close()


@pytest.mark.parametrize("key", ["irregular600", "heavy_rows", "hamming3_a0.0"])
def test_non_temporal_instantiations(key):
    """The kernels that large batches take (non-temporal message traffic: beyond 384 MiB in flight) on small cases, by the switch F32_NT:
    rows and columns in registers and streamed, DR = 8 and 16, DC = 4 and 8."""
    c = CASES[key]()
    eng = _engine(c)
    eng.set_debug_switch("F32_NT", 1)
    with launch_util.launch_log() as log:
        got = eng.decode_batch(c["synd"])
    _same(got, fu.expected(key, c, np.float32), f"{key}/non-temporal")
    eng.close()
    # <DR, NT = 1> and <DC, NT = 1> ran, and no temporal instantiation beside them (host_f32.h: pick_f32)
    hh = sp.csr_matrix(c["h"])
    dr = 8 if int(hh.sum(axis=1).max()) <= 8 else 16
    dc = 4 if int(hh.sum(axis=0).max()) <= 4 else 8
    assert launch_util.of(log, "bp_f32_check_kernel") == [f"bp_f32_check_kernel<{dr}, 1>"], sorted(log)
    assert launch_util.of(log, "bp_f32_bit_kernel") == [f"bp_f32_bit_kernel<{dc}, 1>"], sorted(log)


def test_pipelined_host_arrays():
    """A batch of host arrays large enough for the pipelined path (pinned chunks of 1 024 rows, three in flight: at least 3 chunks and
    64 MiB of results): the 130 rows of the irregular case over and over -- rows are independent, so row b is row b % 130 of the case."""
    c = fu.irregular_case()
    want = fu.expected("irregular600", c, np.float32)
    reps = 12288 // 130 + 1
    idx = np.arange(12288 + 40) % 130  # (a last chunk that is not whole)
    assert reps and len(idx) * (600 * 9 + 300 + 5) >= (64 << 20)
    eng = _engine(c)
    eng.set_debug_switch("HOST_CHUNK_ROWS", 1024)
    _same(eng.decode_batch(np.ascontiguousarray(c["synd"][idx])), tuple(x[idx] for x in want), "irregular600/pipelined host path")
    eng.close()


def test_irregular_one_iteration():
    c = fu.irregular_case(max_iter=1)
    want = fu.expected("irregular600_it1", c, np.float32)
    assert not want[3].all()
    eng = _engine(c)
    _same(eng.decode_batch(c["synd"]), want, "irregular600/max_iter=1")
    eng.close()


@pytest.mark.parametrize("backend", ["cython", "ctypes"])
def test_irregular_single_decode(backend):
    """decode(): one row through the batch kernels (the resident single-decode path is float64 only); rows are independent, so the
    expectation is the batch's row."""
    c = fu.irregular_case()
    want = fu.expected("irregular600", c, np.float32)
    d = _decoder(c, backend)
    for row in (0, int(np.flatnonzero(~want[3])[0])):
        out = d.decode(c["synd"][row])
        _same((out[None, :], d.log_prob_ratios[None, :], np.array([d.iter]), np.array([d.converge])),
              tuple(x[row:row + 1] for x in want), f"irregular600/decode row {row}/{backend}")
    eng = _engine(c)
    _same(eng.decode_batch(c["synd"][:1]), tuple(x[:1] for x in want), "irregular600/B=1")
    eng.close()


@pytest.mark.parametrize("osd_method,osd_order,code", [("osd_0", 0, 1), ("osd_cs", 4, 3)])
def test_bposd_on_widened_posteriors(oracle_built, osd_method, osd_order, code):
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
        got = d.decode_batch(c["synd"])
        _same((got, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), _shortcut((want, llr32, it32, cv32), c["synd"]), f"bb144/{osd_method}/{backend}")
    row = int(np.flatnonzero(~cv32)[0])
    assert np.array_equal(d.decode(c["synd"][row]), want[row]), "BpOsdDecoder.decode in float32"


def test_back_to_float64_reproduces_the_fixture():
    from ldpc_amd.bp_decoder import BpDecoder
    g = load_case("c5_bb144_ms50_p050")
    d = BpDecoder(g["h"], error_channel=list(g["channel_probs"]), max_iter=g["max_iter"], bp_method="minimum_sum",
                  ms_scaling_factor=g["ms_scaling_factor"], input_vector_type="syndrome")
    d.message_dtype = "float32"
    d.decode_batch(g["syndromes"])
    llr32 = d.log_prob_ratios_batch.copy()
    assert np.array_equal(llr32, llr32.astype(np.float32).astype(np.float64)), "float32 mode hands out widened float32 values"
    d.message_dtype = "float64"
    dec = d.decode_batch(g["syndromes"])
    nz = g["syndromes"].any(axis=1)
    assert np.array_equal(dec[nz], g["decoding"][nz]) and np.array_equal(d.converge_batch[nz], g["converge"][nz])
    assert np.array_equal(d.iter_batch[nz], g["iterations"][nz])
    rows = np.flatnonzero(nz[:len(g["llr"])])
    assert bits_equal(d.log_prob_ratios_batch[rows], g["llr"][rows]), "float64 after float32: the fixture's bits"


def test_c_abi_refusals_and_setter():
    from ldpc_amd import _lib
    c = fu.small_case("hamming3", 0.625)
    lib = _lib.load()
    eng = _engine(c, method=0)  # product-sum
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
    assert lib.ldpc_hip_bp_set_message_dtype(eng._h, 2) == -1 and b"message dtype" in lib.ldpc_hip_last_error()
    assert lib.ldpc_hip_bp_get_message_dtype(eng._h) == 1
    small = eng.workspace_bytes(640)
    eng.set_message_dtype("float64")
    assert lib.ldpc_hip_bp_get_message_dtype(eng._h) == 0 and small < eng.workspace_bytes(640)
    eng.close()


def test_close_frees_every_device_buffer():
    """As tests/test_gpu_buffer_leak.py: the library's own count of the bytes its buffers hold."""
    from ldpc_amd import _lib
    c = fu.irregular_case()
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    eng = _engine(c)
    eng.decode_batch(c["synd"])
    eng.set_osd(1, 0)
    eng.decode_batch(c["synd"], osd=True)
    during = held()
    eng.close()
    after = held()
    print(f"float32: device buffer bytes before {before}, with the engine {during}, after close {after}")
    assert during > before and after == before, f"{after - before} bytes of device buffers outlive the handle"


# ---- 70 tiles: looping kernels, the second chunk of the tile list, the early stop ----------------------------------------------------
def _poisoned(b, n, want_llr=True):
    """Output tensors no decode leaves as they are: 0xFF bytes (decisions and flags are 0 / 1, iteration counts positive), NaN."""
    import torch
    return (torch.full((b, n), 0xFF, dtype=torch.uint8, device="cuda"),
            torch.full((b, n), float("nan"), dtype=torch.float64, device="cuda") if want_llr else None,
            torch.full((b,), -1, dtype=torch.int32, device="cuda"), torch.full((b,), 0xFF, dtype=torch.uint8, device="cuda"))


def _decode_poisoned(eng, synd, want, what, want_llr=True):
    """decode_batch on CUDA tensors (one device chunk unless max_chunk_tiles says otherwise) into poisoned buffers, against ``want``."""
    import torch
    assert not np.isnan(want[1]).any() and want[2].min() >= 1, "the poison must differ from every expected value"
    out = _poisoned(len(synd), want[0].shape[1], want_llr)
    got = eng.decode_batch(synd, want_llr=want_llr, out=out)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, out))
    dec, llr, it, cv = (None if x is None else x.cpu().numpy() for x in got)
    if not want_llr:
        assert llr is None
        llr = want[1]
    assert set(np.unique(cv).tolist()) <= {0, 1}, f"{what}: converge flags that were never written"
    _same((dec, llr, it, cv), want, what)


def _switches(eng, grid_rows=None, nodes=None, nt=None):
    for name, value in (("F32_GRID_ROWS", grid_rows), ("SPREAD_NODES", nodes), ("F32_NT", nt)):
        if value is not None:
            eng.set_debug_switch(name, value)


# (grid rows, nodes per wavefront, F32_NT, want_llr): the full product of rows x nodes; F32_NT = 1 and want_llr = False on two of them each
_LOOP_CASES = [(None, 1, None, True), (None, 4, None, False), (None, 16, 1, True),
               (1, 1, None, True), (1, 4, None, True), (1, 16, None, True),
               (3, 1, None, False), (3, 4, 1, True), (3, 16, None, True),
               (64, 1, None, True), (64, 4, None, True), (64, 16, None, True)]


@pytest.mark.parametrize("grid_rows,nodes,nt,want_llr", _LOOP_CASES,
                         ids=[f"rows{g}-nodes{k}" + ("-nt" if nt else "") + ("" if w else "-nollr") for g, k, nt, w in _LOOP_CASES])
def test_tile_list_loops_and_compaction(grid_rows, nodes, nt, want_llr):
    """The standard schedule (70 tiles, B = 4 423; tiles end at iterations 2 ... 12 and 16 in both chunks of the list) with 1, 3 (70 slots
    leave a remainder) and 64 (only rows 0 ... 5 loop twice) workgroup rows and all 70; 16 nodes per wavefront make 64 per workgroup against
    m = 300, n = 600, so the last workgroup of each pass is partial."""
    import torch
    case, idx, synd, want = fu.standard_schedule()
    eng = _engine(case)
    _switches(eng, grid_rows, nodes, nt)
    _decode_poisoned(eng, torch.as_tensor(synd, device="cuda"), want, f"standard schedule/rows {grid_rows}/nodes {nodes}/nt {nt}", want_llr)
    eng.close()


def test_tile_list_in_several_chunks_and_after_a_larger_batch():
    """Chunks of 33, 33 and 4 tiles, each with its own list, counters, flag sequence number and compactions; then 3 tiles on the same
    engine (nothing of the larger decode's list, state or counters may be read), then the 70 again -- that time with 4 workgroup rows."""
    import torch
    case, idx, synd, want = fu.standard_schedule()
    s = torch.as_tensor(synd, device="cuda")
    eng = _engine(case)
    eng.set_tuning(max_chunk_tiles=33)
    _decode_poisoned(eng, s, want, "standard schedule/chunks of 33 tiles")
    _decode_poisoned(eng, s[:192].contiguous(), tuple(x[:192] for x in want), "its first 3 tiles after the 70")
    eng.set_debug_switch("F32_GRID_ROWS", 4)
    _decode_poisoned(eng, s, want, "standard schedule/chunks of 33 tiles again, 4 rows")
    eng.close()


@pytest.mark.parametrize("grid_rows", [None, 2])
@pytest.mark.parametrize("code,alpha", [("hamming3", 0.625), ("rep5", 0.0)])
def test_edge_values_across_the_second_list_chunk(code, alpha, grid_rows):
    """Priors of +-inf and 0, syndrome bytes 2 and 3 and an all-zero row (not short-cut by the engine) in 70 tiles: tiles 1, 4, 7, ... end
    at once, the others run to max_iter, so the first compaction moves running tiles from the second chunk of the list forward."""
    import torch
    case, idx, synd, want = fu.edge_values_batch(code, alpha)
    eng = _engine(case)
    _switches(eng, grid_rows)
    _decode_poisoned(eng, torch.as_tensor(synd, device="cuda"), want, f"{code} a = {alpha} x 70 tiles/rows {grid_rows}")
    eng.close()


def test_large_max_iter_stops_queueing_rounds_f32():
    """As tests/test_gpu_long_max_iter.py for the FP64 route: the round loop of host_f32.h looks at the host-mapped flag before it queues a
    round.  The standard schedule on rows that all converge (the slowest at iteration 12) with max_iter = 200 000 gives what 16 give, and
    its second call costs at most 1.5 s more (that test's margin; without the look the host queues 800 000 launches: several seconds).
    Measured on one MI355X: 0.0011 s at 16 and 0.0015 s at 200 000; 2.40 s at 200 000 with the look taken out."""
    import torch
    case, idx, synd, want16 = fu.standard_schedule(converging_only=True)
    rows, huge = fu.converging_rows_expected(200000)
    pos = np.searchsorted(rows, idx)
    assert np.array_equal(rows[pos], idx)
    want = tuple(x[pos] for x in huge)
    assert want[3].all() and int(want[2].max()) == 12
    assert all(np.array_equal(a, b) for a, b in zip(want[:1] + want[2:], want16[:1] + want16[2:])) and bits_equal(want[1], want16[1])
    s = torch.as_tensor(synd, device="cuda")
    timings = {}
    for max_iter in (16, 200000):
        eng = _engine(dict(case, max_iter=max_iter))
        _decode_poisoned(eng, s, want, f"converging schedule/max_iter {max_iter}, first call")
        out = _poisoned(len(synd), 600)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.decode_batch(s, out=out)
        torch.cuda.synchronize()
        timings[max_iter] = time.perf_counter() - t0
        _same(tuple(x.cpu().numpy() for x in out), want, f"converging schedule/max_iter {max_iter}, second call")
        eng.close()
    print(f"float32 early stop: second call {timings[16]:.4f} s at max_iter 16, {timings[200000]:.4f} s at max_iter 200 000")
    assert timings[200000] < timings[16] + 1.5, timings
