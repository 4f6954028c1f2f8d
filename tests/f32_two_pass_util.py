"""What the tests of the float32 two-pass decode share (tests/test_f32_two_pass_cases.py on the CPU, tests/test_gpu_f32_two_pass.py on the
device): the batches -- rows drawn by index from the 130 rows of ``f32_util.irregular_case()``, so the expectation is the restatement's
rows and a large batch costs no CPU time --, how many rows a first pass of k1 iterations leaves, the pricing of
``stream_first_pass_length`` (csrc/host_handle.h) restated on a histogram, and decodes into poisoned buffers."""
from __future__ import annotations

import functools

import numpy as np

import f32_util as fu
from oracle import bits_equal

MIN_TILES_SWITCH = "F32_REPACK_MIN_TILES"
GATHER = "bp_f32_gather_lanes_kernel"

BIG_FINISH = tuple([16] * 150 + [3, 5, 8, 12] * 10 + [16] * 10)
BIG_LAST_ROWS = 23


@functools.lru_cache(maxsize=None)
def big_schedule():
    """-> (case, idx, syndromes, expectation): 200 tiles, the last of 23 rows (B = 12 759), most of which hold an unconverged row -- a
    first pass of 3 iterations leaves more than 64 tiles' worth of rows, so the second pass's tile list has a second chunk."""
    case = fu.irregular_case()
    want = fu.expected("irregular600", case, np.float32)
    idx, synd = fu.scheduled_batch(case, want, BIG_FINISH, BIG_LAST_ROWS, 7)
    return case, idx, synd, tuple(x[idx] for x in want)


def rows_left(want, k1, max_iter):
    """Rows still decoding after ``k1`` iterations: the second pass's rows."""
    return int((fu.row_end_iterations(want, max_iter) > k1).sum())


def histogram(want):
    """What iteration_histogram_kernel leaves: bin j = rows that converged after exactly j iterations (capped at 255), bin 0 = the rest."""
    it, cv = np.asarray(want[2], np.int64), np.asarray(want[3], bool)
    return np.bincount(np.where(cv, np.clip(it, 1, 255), 0), minlength=256).astype(np.float64)


def first_pass_length(hist, max_iter, gather_cost=0.25):
    """-> (k1, plain, best): the pricing of ``stream_first_pass_length`` in tile-iterations per tile -- F(j) = share converged within j
    iterations; plain = sum_j (1 - F(j-1)^64); a cut at k pays the prefix, the gather (``gather_cost`` x (1 + live)) + 0.1, and ``live`` x
    the same sum over the rows alive after k; cuts with k < 2 or more than 0.6 alive are not priced; it must win by 3 %."""
    full, top = int(max_iter), min(int(max_iter), 255)
    total = float(hist.sum())
    F = np.concatenate(([0.0], np.cumsum(hist[1:top + 1]) / total))
    Fj = lambda j: F[min(j, top)]  # noqa: E731
    runs = lambda j: 1.0 - Fj(j - 1) ** 64  # noqa: E731
    plain = sum(runs(j) for j in range(1, full + 1))
    best, best_k, prefix = plain, 0, 0.0
    for k in range(1, min(full - 1, top) + 1):
        prefix += runs(k)
        live = 1.0 - Fj(k)
        if k < 2 or live <= 0.0 or live > 0.6:
            continue
        rest = sum(1.0 - max((Fj(j - 1) - Fj(k)) / live, 0.0) ** 64 for j in range(k + 1, full + 1))
        cost = prefix + gather_cost * (1.0 + live) + 0.1 + live * rest
        if cost < best:
            best, best_k = cost, k
    return (best_k if best < 0.97 * plain else 0), plain, best


def engine(case, min_tiles=2, repack=None, **switches):
    from ldpc_amd.engine import HipBpEngine
    h = case["h"]
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], case["probs"], case["max_iter"], 1, case["alpha"])
    eng.set_message_dtype("float32")
    if min_tiles is not None:
        eng.set_debug_switch(MIN_TILES_SWITCH, min_tiles)
    for name, value in switches.items():
        if value is not None:
            eng.set_debug_switch(name, value)
    if repack is not None:
        eng.set_repack(repack)
    return eng


def same(got, want, what):
    dec, llr, it, cv = got
    print(f"{what}: {int(np.count_nonzero(np.asarray(dec) != want[0]))} decisions, {int(np.count_nonzero(np.asarray(cv, bool) != want[3]))} flags, "
          f"{int(np.count_nonzero(np.asarray(it) != want[2]))} iteration counts differ")
    assert np.array_equal(np.asarray(dec), want[0]), f"{what}: hard decisions"
    assert np.array_equal(np.asarray(cv, bool), want[3]), f"{what}: converge flags"
    assert np.array_equal(np.asarray(it), want[2]), f"{what}: iteration counts"
    assert bits_equal(np.asarray(llr), want[1]), f"{what}: log-ratios differ in some bit"


def poisoned(b, n, want_llr=True):
    """Output tensors no decode leaves as they are: 0xFF bytes (decisions and flags are 0 / 1, iteration counts positive), NaN."""
    import torch
    return (torch.full((b, n), 0xFF, dtype=torch.uint8, device="cuda"),
            torch.full((b, n), float("nan"), dtype=torch.float64, device="cuda") if want_llr else None,
            torch.full((b,), -1, dtype=torch.int32, device="cuda"), torch.full((b,), 0xFF, dtype=torch.uint8, device="cuda"))


def decode_poisoned(eng, synd, want, what, want_llr=True, **kw):
    """decode_batch on a CUDA tensor into poisoned buffers, synchronised, against ``want`` (None: no comparison) -> the outputs as arrays."""
    import torch
    out = poisoned(len(synd), eng.n, want_llr)
    got = eng.decode_batch(synd, want_llr=want_llr, out=out, **kw)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, out))
    dec, llr, it, cv = (None if x is None else x.cpu().numpy() for x in got)
    assert set(np.unique(cv).tolist()) <= {0, 1}, f"{what}: converge flags that were never written"
    if want is not None:
        assert not np.isnan(want[1]).any() and want[2].min() >= 1, "the poison must differ from every expected value"
        same((dec, want[1] if llr is None else llr, it, cv), want, what)
    return dec, llr, it, cv
