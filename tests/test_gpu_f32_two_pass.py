"""The float32 two-pass decode (csrc/host_f32.h: decode_f32_repacked -- a first pass of k1 iterations that keeps its state,
bp_f32_gather_lanes_kernel, a second pass over rows known to the device only) against the float32 restatement (tests/f32_util.py), bit for
bit: decisions, log-ratio bit patterns, iteration counts and flags, into poisoned buffers.  Batches are drawn by index from the 130 rows of
``f32_util.irregular_case()`` (tests/test_f32_two_pass_cases.py pins what each first pass leaves); they are below 512 tiles, so the switch
F32_REPACK_MIN_TILES = 2 lets them be cut.  The order of the second pass's row list depends on atomic arrival, so only counts and results
are asserted, never which rows share a tile of the second pass."""
import time

import numpy as np
import pytest

import f32_two_pass_util as tu
import f32_util as fu
import launch_util
from oracle import bits_equal

pytestmark = pytest.mark.gpu


def _cuda(synd):
    import torch
    return torch.as_tensor(synd, device="cuda")


def _two_pass(eng, s, want, what, want_llr=True, ran=True, **kw):
    with launch_util.launch_log() as log:
        got = tu.decode_poisoned(eng, s, want, what, want_llr, **kw)
    (launch_util.assert_ran if ran else launch_util.assert_not_ran)(log, tu.GATHER)
    return got, log


@pytest.mark.parametrize("want_llr", [True, False], ids=["llr", "nollr"])
@pytest.mark.parametrize("k1", [2, 3, 4, 5, 8, 15])
def test_forced_first_pass_on_the_standard_schedule(k1, want_llr):
    """A forced cut after k1 iterations, both parities; 15 leaves a second pass of one iteration.  63 / 47 / 31 / 15 / 5 / 4 second-pass
    tiles, every last one partial."""
    case, idx, synd, want = fu.standard_schedule()
    eng = tu.engine(case, repack=k1)
    _, log = _two_pass(eng, _cuda(synd), want, f"standard schedule/k1 {k1}/llr {want_llr}", want_llr)
    eng.close()
    assert log[tu.GATHER] == 1, log
    assert log["bp_f32_state_init_kernel"] == 2 and log["bp_f32_init_kernel"] == 1, "two passes, one message initialisation"


@pytest.mark.parametrize("k1", [0, 1, 16, 40])
def test_first_pass_lengths_that_decode_plainly(k1):
    """0 is off; 1 < 2 and 16, 40 >= max_iter are no first pass: the plain decode, same bits, no gather."""
    case, idx, synd, want = fu.standard_schedule()
    eng = tu.engine(case, repack=k1)
    _, log = _two_pass(eng, _cuda(synd), want, f"standard schedule/k1 {k1} (plain)", ran=False)
    eng.close()
    assert log["bp_f32_state_init_kernel"] == 1, log


@pytest.mark.parametrize("switch,value", [("F32_GRID_ROWS", 1), ("F32_GRID_ROWS", 3), ("SPREAD_NODES", 16), ("F32_NT", 1)])
@pytest.mark.parametrize("k1", [3, 4])
def test_forced_first_pass_under_each_switch(k1, switch, value):
    """Grids of 1 and 3 workgroup rows loop over a second pass of 47 / 31 tiles (3 leaves a remainder); 16 nodes per wavefront leave the
    last workgroup of each pass partial (m = 300, n = 600 against 64 per workgroup); F32_NT = 1 runs the non-temporal instantiations."""
    case, idx, synd, want = fu.standard_schedule()
    eng = tu.engine(case, repack=k1, **{switch: value})
    _, log = _two_pass(eng, _cuda(synd), want, f"standard schedule/k1 {k1}/{switch} = {value}")
    eng.close()
    if switch == "F32_NT":  # (both passes: no temporal instantiation beside the non-temporal ones)
        dr = 8 if int(case["h"].sum(axis=1).max()) <= 8 else 16
        dc = 4 if int(case["h"].sum(axis=0).max()) <= 4 else 8
        assert launch_util.of(log, "bp_f32_check_kernel") == [f"bp_f32_check_kernel<{dr}, 1>"], sorted(log)
        assert launch_util.of(log, "bp_f32_bit_kernel") == [f"bp_f32_bit_kernel<{dc}, 1>"], sorted(log)


@pytest.mark.parametrize("grid_rows", [None, 2])
@pytest.mark.parametrize("k1", [3, 4])
def test_big_schedule_second_list_beyond_64_entries(k1, grid_rows):
    """200 tiles; the second pass has 130 / 83 tiles, so its list has a second chunk of 64 and its compactions (every 4 rounds of the pass)
    move running tiles forward across it."""
    case, idx, synd, want = tu.big_schedule()
    eng = tu.engine(case, repack=k1, F32_GRID_ROWS=grid_rows)
    _, log = _two_pass(eng, _cuda(synd), want, f"big schedule/k1 {k1}/rows {grid_rows}")
    eng.close()
    # compactions: the first pass has fewer than 5 rounds (none), the second 16 - k1 rounds: after its 4th, 8th and 12th
    assert log["bp_f32_compact_kernel"] == (16 - k1 - 1) // 4, log


@pytest.mark.parametrize("code,alpha", [("hamming3", 0.625), ("rep5", 0.0)])
def test_edge_values_carried_into_the_second_pass(code, alpha):
    """Priors of +-inf and 0, syndrome bytes 2 and 3 (rows that never converge: in every second pass, re-packed through the row list) and an
    all-zero row, cut after 2 iterations.  The per-pass kernels on a code the on-chip kernels would take: F32_ONCHIP = 0."""
    case, idx, synd, want = fu.edge_values_batch(code, alpha)
    if case["max_iter"] < 8:  # (the two-pass decode needs 8 iterations: the case's rows with more of them)
        case = dict(case, max_iter=8)
        base = fu.min_sum_restatement(case["h"], case["probs"], case["synd"], 8, case["alpha"], np.float32)
        want = tuple(x[idx] for x in base)
    eng = tu.engine(case, repack=2, F32_ONCHIP=0)
    _two_pass(eng, _cuda(synd), want, f"{code} a = {alpha} x 70 tiles/k1 2")
    eng.close()


def test_second_pass_without_a_row_stops_queueing_rounds():
    """Every row of the converging schedule is done after 12 iterations, so a first pass of 12 leaves the second pass nothing:
    bp_f32_state_init_kernel reports the decode finished itself and the host stops queueing rounds -- at max_iter = 200 000 as at 16, same
    bits, the second call at most 1.5 s slower (the margin of test_large_max_iter_stops_queueing_rounds_f32, which records 2.4 s without
    the early stop).  Measured on one MI355X: 0.0011 s at 16 and 0.0015 s at 200 000."""
    import torch
    case, idx, synd, want16 = fu.standard_schedule(converging_only=True)
    rows, huge = fu.converging_rows_expected(200000)
    pos = np.searchsorted(rows, idx)
    want = tuple(x[pos] for x in huge)
    assert all(np.array_equal(a, b) for a, b in zip(want[:1] + want[2:], want16[:1] + want16[2:])) and bits_equal(want[1], want16[1])
    s = _cuda(synd)
    timings = {}
    for max_iter in (16, 200000):
        eng = tu.engine(dict(case, max_iter=max_iter), repack=12)
        _two_pass(eng, s, want, f"converging schedule/k1 12/max_iter {max_iter}, first call")
        out = tu.poisoned(len(synd), 600)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.decode_batch(s, out=out)
        torch.cuda.synchronize()
        timings[max_iter] = time.perf_counter() - t0
        tu.same(tuple(x.cpu().numpy() for x in out), want, f"converging schedule/k1 12/max_iter {max_iter}, second call")
        eng.close()
    print(f"float32 two-pass, empty second pass: second call {timings[16]:.4f} s at max_iter 16, {timings[200000]:.4f} s at max_iter 200 000")
    assert timings[200000] < timings[16] + 1.5, timings


def test_automatic_first_pass_from_the_previous_histogram():
    """set_repack(-1), the default: the first decode on a handle runs plain and leaves its histogram; each decode is synchronised, so the
    next one sees it, prices the standard schedule (cut at 6: tests/test_f32_two_pass_cases.py) and runs two passes.  set_repack(0)
    switches that off."""
    case, idx, synd, want = fu.standard_schedule()
    s = _cuda(synd)
    eng = tu.engine(case, repack=-1)
    logs = []
    for i in range(3):
        with launch_util.launch_log() as log:
            tu.decode_poisoned(eng, s, want, f"standard schedule/automatic, decode {i}")
        logs.append(log)
    launch_util.assert_not_ran(logs[0], tu.GATHER)  # (no histogram yet)
    launch_util.assert_ran(logs[-1], tu.GATHER)
    eng.set_repack(0)
    _two_pass(eng, s, want, "standard schedule/automatic, then off", ran=False)
    eng.close()


def test_chunked_batches_decode_plainly_and_smaller_batches_read_nothing_stale():
    """The compaction needs the whole batch's message state resident: with chunks of 33 tiles set_repack(4) decodes plainly.  Then, without
    the limit, the first 3 tiles and all 70 with k1 = 4 on the same engine: nothing of the larger decode's row list, tile states or
    counters may be read by the smaller, and the other way round."""
    case, idx, synd, want = fu.standard_schedule()
    s = _cuda(synd)
    eng = tu.engine(case, repack=4)
    eng.set_tuning(max_chunk_tiles=33)
    _two_pass(eng, s, want, "standard schedule/k1 4/chunks of 33 tiles (plain)", ran=False)
    eng.set_tuning(max_chunk_tiles=0)
    _two_pass(eng, s, want, "standard schedule/k1 4/one chunk")
    _two_pass(eng, s[:192].contiguous(), tuple(x[:192] for x in want), "its first 3 tiles/k1 4, after the 70")
    _two_pass(eng, s, want, "standard schedule/k1 4/one chunk, after the 3")
    eng.close()


def test_one_handle_across_message_dtypes():
    """float32 two-pass, float64, float32 two-pass on one handle: the workspace changes its element type between the decodes.  (The
    float64 decode of 70 tiles is below its own 512-tile rule either way; it is compared with set_repack(0) on the same handle.)"""
    case, idx, synd, want = fu.standard_schedule()
    s = _cuda(synd)
    eng = tu.engine(case, repack=4)
    _two_pass(eng, s, want, "float32 two-pass, first")
    eng.set_message_dtype("float64")
    got64 = tu.decode_poisoned(eng, s, None, "float64 between")
    eng.set_repack(0)
    ref64 = tu.decode_poisoned(eng, s, None, "float64, set_repack(0)")
    tu.same(got64, (ref64[0], ref64[1], ref64[2], ref64[3].astype(bool)), "float64 between two float32 two-pass decodes")
    assert not bits_equal(got64[1], want[1]), "the float64 decode returned float32 posteriors"
    eng.set_repack(4)
    eng.set_message_dtype("float32")
    _two_pass(eng, s, want, "float32 two-pass, after float64")
    eng.close()


def test_bposd0_on_a_two_pass_decode():
    """BP + OSD-0 (bposd_device collects the rows BP left unconverged after decode_device) on a two-pass float32 decode: decisions and
    status bytes equal those of the same engine with set_repack(0)."""
    import torch
    case, idx, synd, want = fu.standard_schedule()
    s = _cuda(synd)
    eng = tu.engine(case, repack=0)
    eng.set_osd(1, 0)
    res = {}
    for k1 in (0, 4):
        eng.set_repack(k1)
        with launch_util.launch_log() as log:
            dec, llr, it, cv = tu.decode_poisoned(eng, s, None, f"BP + OSD-0/k1 {k1}", osd=True)
        (launch_util.assert_ran if k1 else launch_util.assert_not_ran)(log, tu.GATHER)
        torch.cuda.synchronize()
        res[k1] = (dec, llr, it, cv, np.asarray(eng.osd_status(len(synd))))
    eng.close()
    assert (res[0][4] != 0).sum() == (~want[3]).sum() > 0 and set(np.unique(res[0][4]).tolist()) <= {0, 1, 2}
    assert np.array_equal(res[4][0], res[0][0]), "decisions after OSD-0"
    assert np.array_equal(res[4][4], res[0][4]), "OSD status bytes"
    assert np.array_equal(res[4][2], res[0][2]) and np.array_equal(res[4][3], res[0][3]) and bits_equal(res[4][1], res[0][1])
    assert np.array_equal(res[4][2], want[2]) and bits_equal(res[4][1], want[1]), "BP's own outputs: the restatement's"
    conv = want[3]
    assert np.array_equal(res[4][0][conv], want[0][conv])


def test_close_frees_every_device_buffer_after_a_two_pass_decode():
    """As tests/test_gpu_buffer_leak.py: the library's own count of the bytes its buffers hold (row list, counters, scratch flags and
    iteration counts, histogram included)."""
    from ldpc_amd import _lib
    case, idx, synd, want = fu.standard_schedule()
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    eng = tu.engine(case, repack=4)
    with launch_util.launch_log() as log:
        eng.decode_batch(synd, want_llr=False)
    launch_util.assert_ran(log, tu.GATHER)
    eng.set_osd(1, 0)
    eng.decode_batch(synd, osd=True)
    during = held()
    eng.close()
    after = held()
    print(f"float32 two-pass: device buffer bytes before {before}, with the engine {during}, after close {after}")
    assert during > before and after == before, f"{after - before} bytes of device buffers outlive the handle"
