"""NumPy restatement of memory min-sum BP (``ldpc_hip_bp_set_memory``) -- the contract the device reproduces bit for
bit -- and the cases the CPU and GPU tests share.

``min_sum_memory_restatement`` is ``f32_util.min_sum_restatement`` at ``np.float64`` with ONE change: the bit pass of column j starts its
forward sum from

    prior_it[b][j] = L0[j]                              if gamma[j] == 0.0   (a select, no arithmetic)
                   = a[j] + gamma[j] * M_prev[b][j]     otherwise,           a[j] = (1.0 - gamma[j]) * L0[j]   (two roundings)

instead of ``L0[j]``; ``M_prev`` is the posterior (the forward sum's end value) the previous iteration's bit pass computed for that row,
``L0[j]`` before the first.  The product is rounded, then the sum (NumPy rounds every elementwise operation once).  ``M`` keeps evolving for
every row; a converged row's OUTPUTS are frozen as in the plain decode.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

import f32_util as fu


def memory_a(channel_probs, gamma):
    """``a[j]``: ``L0[j]`` where ``gamma[j] == 0`` (what ``1.0 * L0`` is, infinities included), else ``(1.0 - gamma[j]) * L0[j]``."""
    l0 = fu.priors_f64(channel_probs)
    g = np.asarray(gamma, np.float64)
    with np.errstate(all="ignore"):
        return np.where(g == 0.0, l0, (np.float64(1.0) - g) * l0)


def min_sum_memory_restatement(h, channel_probs, gamma, syndromes, max_iter, ms_scaling_factor):
    """-> (decoding (B, n) uint8, llr (B, n) float64, iterations (B,) int32, converge (B,) bool)."""
    dtype = np.float64
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
    prior = fu.priors_f64(channel_probs).astype(dtype)
    gamma = np.asarray(gamma, np.float64)
    assert gamma.shape == (n,)
    a_mem = memory_a(channel_probs, gamma)
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
    mem = np.tile(prior, (B, 1))  # M: the posterior of the previous iteration, L0 to begin with
    hd = h.toarray().astype(np.int64)
    with np.errstate(all="ignore"):
        for it in range(1, int(max_iter) + 1):
            alpha = dt(1.0 - 2.0 ** (-it) if ms_scaling_factor == 0.0 else float(ms_scaling_factor))
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
                if gamma[j] == 0.0:
                    temp = np.full(B, prior[j], dtype)
                else:
                    temp = a_mem[j] + gamma[j] * mem[:, j]  # the product rounded, then the sum
                for p in range(col_ptr[j], col_ptr[j + 1]):
                    e = order[p]
                    b2c[e] = temp
                    temp = temp + c2b[e]
                llr[:, j] = temp
                dec[:, j] = temp <= 0
            mem = llr.copy()
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
    return dec_out, llr_out, iters, conv


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
GAMMA_PATTERN = (-0.24, 0.0, 0.35, 0.66, 0.125, -0.5)


def mixed_gamma(probs):
    """0.0 on some columns, negative and positive strengths on the others; 0.0 wherever p is 0 or 1 (their priors are infinite), and a
    nonzero strength on every p = 0.5 column (prior +0.0)."""
    probs = np.asarray(probs, np.float64)
    g = np.array([GAMMA_PATTERN[j % len(GAMMA_PATTERN)] for j in range(len(probs))], np.float64)
    g[(probs <= 0.0) | (probs >= 1.0)] = 0.0
    g[(probs == 0.5) & (g == 0.0)] = 0.35
    return g


def drawn_gamma(n, seed):
    """Per-bit strengths drawn from [-0.24, 0.66] with a fixed seed."""
    return np.random.default_rng(seed).uniform(-0.24, 0.66, size=n)


_EXPECT: dict = {}


def expected(key, case, gamma):
    """The memory restatement's outputs for (case, gamma), computed once per key and shared (read-only)."""
    if key not in _EXPECT:
        out = min_sum_memory_restatement(case["h"], case["probs"], gamma, case["synd"], case["max_iter"], case["alpha"])
        for x in out:
            x.setflags(write=False)
        _EXPECT[key] = out
    return _EXPECT[key]


def plain(key, case):
    """The plain FP64 restatement of a case (f32_util.min_sum_restatement), computed once per key."""
    k = ("plain", key)
    if k not in _EXPECT:
        _EXPECT[k] = fu.min_sum_restatement(case["h"], case["probs"], case["synd"], case["max_iter"], case["alpha"], np.float64)
    return _EXPECT[k]


def assert_shows_something(want, plain_out, max_iter, what):
    """What every GPU test asserts on the restatement's own output: a row that converges before max_iter, a row that does not converge, and a
    row whose result differs from the plain decode's -- otherwise the comparison shows nothing."""
    dec, llr, it, cv = want
    assert (cv & (it < max_iter)).any(), f"{what}: no row converges before max_iter"
    assert (~cv).any(), f"{what}: every row converges"
    differs = (dec != plain_out[0]).any(axis=1) | (it != plain_out[2]) | (cv != plain_out[3]) | \
        (llr.view(np.uint64) != np.ascontiguousarray(plain_out[1]).view(np.uint64)).any(axis=1)
    assert differs.any(), f"{what}: the memory decode equals the plain decode on every row"


@functools.lru_cache(maxsize=None)
def edge_case(code):
    """The lane = edge cases: (h, p) with B = 3000 syndromes at a noise where min-sum 12 converges on some rows and not on others; the
    B = 70 tests take the first 70 rows.  surface5: bp_edge_mem_kernel; bb144: bp_edge8_mem_kernel<., 3>; hgp_hamming3: <., 4>."""
    from ldpc_amd import codes
    from ldpc_amd.codes import synthetic
    h, p, seed = {"surface5": (lambda: synthetic.rotated_surface_code_x(5), 0.09, 31),
                  "bb144": (lambda: synthetic.bivariate_bicycle_hx(), 0.05, 32),
                  "hgp_hamming3": (lambda: synthetic.hypergraph_product_hx(codes.hamming_code(3)), 0.05, 33)}[code]
    h = sp.csr_matrix(h())
    h.eliminate_zeros()  # (the hypergraph product stores explicit zeros; the decoders drop them on ingest, an engine takes the arrays as they are)
    h.sort_indices()
    return dict(h=h, probs=np.full(h.shape[1], p), synd=fu.bsc_syndromes(h, 3000, p, seed), max_iter=12, alpha=0.625)


def first_rows(case, rows):
    c = dict(case)
    c["synd"] = np.ascontiguousarray(case["synd"][:rows])
    return c
