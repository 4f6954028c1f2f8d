"""NumPy restatement of parallel (flooding) min-sum BP, parametrised by the message dtype -- the contract of the float32 message mode
("float32 messages") with explicit per-operation types, and the cases the CPU and GPU tests share.

At ``np.float64`` it performs the operations of ``oracle/bp_oracle.c`` (bp.hpp:192-325) in their order and must equal the oracle bit
for bit (tests/test_f32_restatement.py); at ``np.float32`` it is what the device must compute (tests/test_gpu_f32.py):

* priors: ``log((1 - p) / p)`` in FP64 with the host libm, rounded once to ``dtype``;
* check pass: per edge the minimum of ``|bit_to_check|`` over the row's other entries (``finfo(dtype).max`` for none), sign from the
  others' signs and the syndrome byte, times ``alpha`` in one multiply; ``alpha`` formed in FP64, rounded once to ``dtype``;
* bit pass: forward partial sums from the prior, backward partial sums from 0, one ``dtype`` addition each, the reference's operand order;
* posterior = the forward sum, decision ``posterior <= 0``; a row whose candidate syndrome equals its syndrome BYTES freezes its outputs.

Every array below has the message dtype, and NumPy rounds each elementwise operation of two ``dtype`` arrays once to ``dtype``; the
minimum is written with the comparisons of the reference (``a < temp``), which decide NaNs as the kernels do.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import scipy.sparse as sp


def priors_f64(channel_probs):
    """``log((1 - p) / p)`` as upload_priors / bp.hpp:150-151 evaluate it: IEEE division, the host libm's log."""
    p = np.asarray(channel_probs, np.float64)
    with np.errstate(all="ignore"):
        x = (1.0 - p) / p
    out = np.empty(len(p), np.float64)
    for j, v in enumerate(x):
        v = float(v)
        out[j] = -math.inf if v == 0.0 else math.inf if v == math.inf else math.nan if (v != v or v < 0) else math.log(v)
    return out


def min_sum_restatement(h, channel_probs, syndromes, max_iter, ms_scaling_factor, dtype):
    """-> (decoding (B, n) uint8, llr (B, n) float64 = the ``dtype`` posteriors widened, iterations (B,) int32, converge (B,) bool)."""
    h = sp.csr_matrix(h)
    h.sort_indices()
    m, n = h.shape
    row_ptr, col_idx = h.indptr, h.indices
    nnz = len(col_idx)
    edge_row = np.repeat(np.arange(m), np.diff(row_ptr))
    order = np.lexsort((edge_row, col_idx))  # column by column, rows ascending: CSR edge ids
    col_ptr = np.concatenate(([0], np.cumsum(np.bincount(col_idx, minlength=n)))).astype(np.int64)
    dt = np.dtype(dtype).type
    big = dt(np.finfo(dtype).max)
    synd = np.ascontiguousarray(syndromes, np.uint8)
    B = synd.shape[0]
    prior = priors_f64(channel_probs).astype(dtype)  # one rounding
    b2c = np.empty((nnz, B), dtype)
    c2b = np.zeros((nnz, B), dtype)
    for e in range(nnz):
        b2c[e] = prior[col_idx[e]]
    dec_out = np.zeros((B, n), np.uint8)
    llr_out = np.zeros((B, n), dtype)
    iters = np.zeros(B, np.int32)
    conv = np.zeros(B, bool)
    dec = np.zeros((B, n), np.uint8)
    llr = np.zeros((B, n), dtype)
    hd = h.toarray().astype(np.int64)
    with np.errstate(all="ignore"):
        for it in range(1, int(max_iter) + 1):
            alpha = dt(1.0 - 2.0 ** (-it) if ms_scaling_factor == 0.0 else float(ms_scaling_factor))  # FP64, then one rounding
            for i in range(m):
                lo, hi = row_ptr[i], row_ptr[i + 1]
                total = synd[:, i].astype(np.int64)
                temp = np.full(B, big, dtype)
                for e in range(lo, hi):
                    total = total + (b2c[e] <= 0)
                    c2b[e] = temp
                    a = np.abs(b2c[e])
                    temp = np.where(a < temp, a, temp)
                temp = np.full(B, big, dtype)
                for e in range(hi - 1, lo - 1, -1):
                    sgn = total + (b2c[e] <= 0)
                    mag = np.where(temp < c2b[e], temp, c2b[e])
                    c2b[e] = mag * np.where(sgn % 2 == 0, alpha, -alpha).astype(dtype)
                    a = np.abs(b2c[e])
                    temp = np.where(a < temp, a, temp)
            for j in range(n):
                temp = np.full(B, prior[j], dtype)
                for p in range(col_ptr[j], col_ptr[j + 1]):
                    e = order[p]
                    b2c[e] = temp
                    temp = temp + c2b[e]
                llr[:, j] = temp
                dec[:, j] = temp <= 0
            cand = (dec.astype(np.int64) @ hd.T) & 1
            ok = np.all(cand == synd, axis=1) if m else np.ones(B, bool)
            run = ~conv
            dec_out[run] = dec[run]
            llr_out[run] = llr[run]
            iters[run] = it
            conv |= ok
            if conv.all():
                break
            for j in range(n):
                temp = np.zeros(B, dtype)
                for p in range(col_ptr[j + 1] - 1, col_ptr[j] - 1, -1):
                    e = order[p]
                    b2c[e] = b2c[e] + temp
                    temp = temp + c2b[e]
    assert b2c.dtype == np.dtype(dtype) and c2b.dtype == np.dtype(dtype) and llr.dtype == np.dtype(dtype)
    return dec_out, llr_out.astype(np.float64), iters, conv


# ---- the cases (ISSUE: "smallest shapes that can still go wrong"); built once per process ----------------------------------------------
def bsc_syndromes(h, batch, p, seed):
    rng = np.random.default_rng(seed)
    errors = (rng.random((batch, h.shape[1])) < p).astype(np.uint8)
    return np.ascontiguousarray((errors @ h.T.toarray().astype(np.uint8)) & 1, np.uint8)


def _edge_syndromes(h, batch, seed):
    """Random syndromes with row 5 all zero, a byte 2 in row 9 and a byte 3 in row 66."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, size=(batch, h.shape[0]), dtype=np.uint8)
    s[5] = 0
    s[9, 0] = 2
    s[66, h.shape[0] - 1] = 3
    return s


def _edge_channel(n):
    base = [0.0, 1.0, 0.5, 1e-300, 0.03, 0.2, 0.45, 0.07, 0.11, 0.3]
    return np.array([base[j % len(base)] if j < len(base) else 0.01 + 0.04 * (j % 7) for j in range(n)], np.float64)


@functools.lru_cache(maxsize=None)
def small_case(code, alpha):
    """hamming_code(3) / rep_code(5), B = 70 (64 + 6), non-uniform channel with p = 0, 1, 0.5, 1e-300."""
    from ldpc_amd import codes
    h = sp.csr_matrix({"hamming3": codes.hamming_code(3), "rep5": codes.rep_code(5)}[code])
    probs = _edge_channel(h.shape[1])
    if code == "rep5":
        probs = probs[[4, 0, 3, 2, 1]]  # (five bits: keep every special value)
    return dict(h=h, probs=probs, synd=_edge_syndromes(h, 70, 7), max_iter=12, alpha=alpha)


@functools.lru_cache(maxsize=None)
def degree1_case():
    from golden_util import load_case
    c = load_case("edge_degree1_empty_ms")
    return dict(h=c["h"], probs=c["channel_probs"], synd=c["syndromes"], max_iter=c["max_iter"], alpha=c["ms_scaling_factor"])


@functools.lru_cache(maxsize=None)
def irregular_case(batch=130, max_iter=16):
    from ldpc_amd import codes
    h = codes.irregular_ldpc_code(600, 300, seed=3, col_weights=((2, 0.20), (3, 0.50), (6, 0.15), (8, 0.10), (11, 0.05)))
    return dict(h=sp.csr_matrix(h), probs=np.full(600, 0.03), synd=bsc_syndromes(h, 130, 0.03, 21)[:batch], max_iter=max_iter, alpha=0.625)


@functools.lru_cache(maxsize=None)
def heavy_rows_case():
    """Rows of 20 and 17 entries -- more than the check kernel keeps in registers (16): its two sweeps through memory -- beside rows of 3,
    and columns of 1 ... 5 entries; B = 70."""
    n = 40
    rows = [list(range(0, 20)), list(range(15, 32)), [0, 20, 32, 39], [1, 16, 33, 34], [2, 17, 35, 36, 37, 38], [3, 18, 19, 31]]
    h = sp.lil_matrix((len(rows), n), dtype=np.uint8)
    for i, cols in enumerate(rows):
        h[i, cols] = 1
    h = sp.csr_matrix(h)
    assert int(np.diff(h.indptr).max()) == 20 and int(h.sum(axis=0).min()) >= 1
    probs = 0.02 + 0.01 * (np.arange(n) % 9)
    return dict(h=h, probs=probs, synd=bsc_syndromes(h, 70, 0.06, 13), max_iter=12, alpha=0.75)


@functools.lru_cache(maxsize=None)
def bb144_case():
    from ldpc_amd import codes
    h = sp.csr_matrix(codes.bivariate_bicycle_hx())
    return dict(h=h, probs=np.full(h.shape[1], 0.06), synd=bsc_syndromes(h, 70, 0.06, 5), max_iter=10, alpha=0.625)


_EXPECT: dict = {}


def expected(key, case, dtype):
    """The restatement's outputs for a case, computed once per (key, dtype) and shared (callers must not write to them)."""
    k = (key, np.dtype(dtype).name)
    if k not in _EXPECT:
        _EXPECT[k] = min_sum_restatement(case["h"], case["probs"], case["synd"], case["max_iter"], case["alpha"], dtype)
    return _EXPECT[k]


# ---- a large batch assembled from rows whose float32 outcome is known: which tile ends at which iteration is chosen ------------------
def row_end_iterations(want, max_iter):
    """The iteration at which each row of a restatement result stops occupying its lane: its count, or ``max_iter`` if it never converges."""
    return np.where(want[3], want[2], max_iter).astype(np.int64)


def scheduled_batch(case, want, finish, last_rows, seed):
    """-> (idx, synd[idx]): a batch of ``len(finish)`` tiles of 64 rows (the last of ``last_rows``) whose tile t is drawn, with a seeded
    generator, from the rows of ``case`` that take at most ``finish[t]`` iterations in ``want`` (its restatement outputs), at least one of
    them exactly ``finish[t]`` -- so tile t ends at iteration ``finish[t]``.  ``finish[t] == max_iter`` stands for a tile that holds an
    unconverged row.  Rows are independent: the expectation is ``tuple(x[idx] for x in want)``."""
    rng = np.random.default_rng(seed)
    max_iter = int(case["max_iter"])
    end, conv = row_end_iterations(want, max_iter), np.asarray(want[3], bool)
    idx = []
    for t, f in enumerate(finish):
        rows = last_rows if t == len(finish) - 1 else 64
        pool = np.flatnonzero(end <= f)
        exact = np.flatnonzero(~conv) if f == max_iter else np.flatnonzero(conv & (end == f))
        assert 1 <= rows <= 64 and len(exact), f"tile {t}: no row of the case ends at iteration {f}"
        tile = rng.choice(pool, size=rows)
        tile[rng.integers(rows)] = rng.choice(exact)
        idx.append(tile)
    idx = np.concatenate(idx).astype(np.int64)
    return idx, np.ascontiguousarray(case["synd"][idx])


def tile_end_iterations(want, idx, max_iter):
    """Per tile of 64 rows of ``idx``: the iteration after which the tile is final (the largest of its rows)."""
    end = row_end_iterations(want, max_iter)[idx]
    return np.array([int(end[t:t + 64].max()) for t in range(0, len(idx), 64)])


# The standard schedule: 70 tiles, the last of 7 rows (B = 4 423).  The sorted end iterations below are dealt out by the fixed
# permutation t -> (37 t + 8) mod 70, which puts tiles that end early in both 64-slot chunks of the tile list and between tiles that run to
# the end; tests/test_f32_restatement.py::test_standard_schedule_has_the_properties_the_gpu_tests_rely_on says what that gives.
_STANDARD_LEVELS = [2, 4, 5, 7, 8, 10, 10, 11, 11, 12, 12] + [16] * 59
STANDARD_FINISH = tuple(_STANDARD_LEVELS[(37 * t + 8) % 70] for t in range(70))
STANDARD_LAST_ROWS = 7
COMPACTION_ROUNDS = (4, 8, 12)  # host_f32.h: round >= 4 && round % 4 == 0, 16 iterations


@functools.lru_cache(maxsize=None)
def standard_schedule(converging_only=False, seed=2024):
    """-> (case, idx, syndromes, expectation) of the standard schedule on ``irregular_case()``; ``converging_only``: tiles that would hold
    an unconverged row end with the slowest row that converges instead (iteration 12), so every row of the batch converges."""
    case = irregular_case()
    want = expected("irregular600", case, np.float32)
    finish = STANDARD_FINISH
    if converging_only:
        longest = int(want[2][want[3]].max())
        finish = tuple(min(f, longest) for f in finish)
    idx, synd = scheduled_batch(case, want, finish, STANDARD_LAST_ROWS, seed)
    return case, idx, synd, tuple(x[idx] for x in want)


@functools.lru_cache(maxsize=None)
def edge_values_batch(code, alpha, tiles=70, last_rows=6):
    """-> (case, idx, syndromes, expectation): the 70 rows of ``small_case(code, alpha)`` replicated by index to ``tiles`` tiles, the last
    of ``last_rows`` rows.  Tiles 1, 4, 7, ... hold only rows that converge (within 2 iterations: they end at once); every other tile
    walks through all rows of the case -- the syndrome bytes 2 and 3 and the rows that never converge included -- and runs to ``max_iter``.
    The index strides (37 rows of 70, 1 row of the converging ones) are no multiples of 64, so no tile repeats its neighbour."""
    case = small_case(code, alpha)
    want = expected(f"{code}_a{alpha}", case, np.float32)
    quick = np.flatnonzero(want[3])
    b = np.arange((tiles - 1) * 64 + last_rows, dtype=np.int64)
    idx = np.where((b // 64) % 3 == 1, quick[b % len(quick)], (b * 37) % len(case["synd"]))
    return case, idx, np.ascontiguousarray(case["synd"][idx]), tuple(x[idx] for x in want)


@functools.lru_cache(maxsize=None)
def converging_rows_expected(max_iter):
    """-> (rows, outputs): the rows of ``irregular_case()`` that converge within its 16 iterations, and the float32 restatement of exactly
    those rows with another ``max_iter`` (it stops once all have converged, so a huge ``max_iter`` costs nothing)."""
    case = irregular_case()
    rows = np.flatnonzero(expected("irregular600", case, np.float32)[3])
    return rows, min_sum_restatement(case["h"], case["probs"], case["synd"][rows], max_iter, case["alpha"], np.float32)
