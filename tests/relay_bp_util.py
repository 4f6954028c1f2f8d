"""NumPy restatement of Relay-BP (``ldpc_hip_bp_set_relay``) -- the contract both device routes reproduce bit for bit --
and the cases the CPU and GPU tests share.

Relay-BP chains memory min-sum legs (``mem_bp_util.min_sum_memory_restatement``: minimum-sum, flooding schedule, FP64).  Per syndrome row,
with ``L0`` the prior log-ratios::

    M = L0; best_w = +inf; nsol = 0; total = 0
    for leg l = 0 .. L-1:
        g = gamma[l]; a = mem_bp_util.memory_a(probs, g)
        initial bit-to-check of every entry of column j:
            l == 0: L0[j]
            l  > 0: g[j] == 0 ? L0[j] : a[j] + g[j] * M[j]          (the product rounded, then the sum)
        iterate it = 1 .. leg_iters[l] exactly as the memory decode does (alpha = 1 - 2^-it with the LEG-LOCAL it when the scaling factor
            is 0; the prior is formed from M; stop at the first iteration whose decisions reproduce the syndrome; a syndrome byte > 1
            never converges)
        total += iterations run
        M = the posterior of the last bit pass run
        if the leg converged:
            nsol += 1; w = weight(decisions)
            if w < best_w: best = (decisions, M, w)                  (strict: the first of equal weights stays; NaN never wins)
            if nsol == stop_after: stop
    converge = nsol > 0;  decoding, llr = best if converge else the last leg's last bit pass;  iterations = total

``relay_weight`` is an FP64 sum in one fixed order (see there).  ``memory_leg`` is the loop of ``min_sum_memory_restatement`` with two
additions -- the initial messages and ``M`` may start from a seed -- and is tested against it bit for bit (tests/test_relay_restatement.py).
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

import f32_util as fu
import mem_bp_util as mu


def relay_weight(dec, l0):
    """The weight of decisions ``dec`` ((B, n) or (n,)) under prior log-ratios ``l0`` (n,), in the order every kernel uses:
    ``t[j] = dec[j] ? l0[j] : +0.0`` (a select); ``p[lane] = ((0.0 + t[lane]) + t[lane + 64]) + ...`` for lane = 0 .. 63 over j < n
    ascending; then for s in 1, 2, 4, 8, 16, 32: ``p[lane] = p[lane] + p[lane ^ s]``; the weight is ``p[0]``."""
    dec = np.asarray(dec)
    single = dec.ndim == 1
    dec = np.atleast_2d(dec)
    l0 = np.asarray(l0, np.float64)
    n = dec.shape[1]
    t = np.where(dec != 0, l0[None, :], np.float64(0.0))
    p = np.zeros((dec.shape[0], 64), np.float64)
    with np.errstate(all="ignore"):
        for j0 in range(0, n, 64):
            w = min(64, n - j0)
            p[:, :w] = p[:, :w] + t[:, j0:j0 + w]
        lanes = np.arange(64)
        for s in (1, 2, 4, 8, 16, 32):
            p = p + p[:, lanes ^ s]
    return p[0, 0] if single else p[:, 0].copy()


class _Graph:
    def __init__(self, h):
        h = sp.csr_matrix(h)
        h.sort_indices()
        self.m, self.n = h.shape
        self.row_ptr, self.col_idx = h.indptr, h.indices
        self.nnz = len(self.col_idx)
        edge_row = np.repeat(np.arange(self.m), np.diff(self.row_ptr))
        self.order = np.lexsort((edge_row, self.col_idx))  # column by column, rows ascending: CSR edge ids
        self.col_ptr = np.concatenate(([0], np.cumsum(np.bincount(self.col_idx, minlength=self.n)))).astype(np.int64)
        self.hd_t = h.toarray().astype(np.int64).T


def memory_leg(graph, prior, a_mem, gamma, synd, seed, max_iter, ms_scaling_factor):
    """One memory min-sum decode of ``synd`` (B, m) to ``max_iter`` iterations: ``mem_bp_util.min_sum_memory_restatement``'s loop, started
    from ``seed`` (B, n) -- M, and the initial messages ``gamma[j] == 0 ? prior[j] : a_mem[j] + gamma[j] * seed[b][j]`` -- or, with
    ``seed=None``, from the priors as the memory decode does.  -> (decoding, llr, iterations, converge), a converged row's outputs frozen at
    its convergence iteration."""
    g = graph
    dtype = np.float64
    big = np.float64(np.finfo(dtype).max)
    B = synd.shape[0]
    b2c = np.empty((g.nnz, B), dtype)
    c2b = np.zeros((g.nnz, B), dtype)
    with np.errstate(all="ignore"):
        if seed is None:
            mem = np.tile(prior, (B, 1))
            for e in range(g.nnz):
                b2c[e] = prior[g.col_idx[e]]
        else:
            mem = np.array(seed, dtype)
            for e in range(g.nnz):
                j = g.col_idx[e]
                b2c[e] = prior[j] if gamma[j] == 0.0 else a_mem[j] + gamma[j] * mem[:, j]  # the product rounded, then the sum
    dec_out = np.zeros((B, g.n), np.uint8)
    llr_out = np.zeros((B, g.n), dtype)
    iters = np.zeros(B, np.int32)
    conv = np.zeros(B, bool)
    dec = np.zeros((B, g.n), np.uint8)
    llr = np.zeros((B, g.n), dtype)
    with np.errstate(all="ignore"):
        for it in range(1, int(max_iter) + 1):
            alpha = np.float64(1.0 - 2.0 ** (-it) if ms_scaling_factor == 0.0 else float(ms_scaling_factor))
            for i in range(g.m):
                lo, hi = g.row_ptr[i], g.row_ptr[i + 1]
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
            for j in range(g.n):
                if gamma[j] == 0.0:
                    temp = np.full(B, prior[j], dtype)
                else:
                    temp = a_mem[j] + gamma[j] * mem[:, j]  # the product rounded, then the sum
                for p in range(g.col_ptr[j], g.col_ptr[j + 1]):
                    e = g.order[p]
                    b2c[e] = temp
                    temp = temp + c2b[e]
                llr[:, j] = temp
                dec[:, j] = temp <= 0
            mem = llr.copy()
            cand = (dec.astype(np.int64) @ g.hd_t) & 1
            ok = np.all(cand == synd, axis=1) if g.m else np.ones(B, bool)
            run = ~conv
            dec_out[run] = dec[run]
            llr_out[run] = llr[run]
            iters[run] = it
            conv |= ok
            if conv.all():
                break
            for j in range(g.n):
                temp = np.zeros(B, dtype)
                for p in range(g.col_ptr[j + 1] - 1, g.col_ptr[j] - 1, -1):
                    e = g.order[p]
                    b2c[e] = b2c[e] + temp
                    temp = temp + c2b[e]
    return dec_out, llr_out, iters, conv


def relay_restatement(h, channel_probs, gamma, leg_iters, stop_after, syndromes, ms_scaling_factor, details=False):
    """-> (decoding (B, n) uint8, llr (B, n) float64, iterations (B,) int32, converge (B,) bool); with ``details=True`` a fifth entry, a dict
    of per-row bookkeeping: ``nsol``, ``first_leg`` (leg of the first solution, -1: none), ``replaced`` (times a later solution replaced an
    earlier one), ``best_w``."""
    graph = _Graph(h)
    gamma = np.atleast_2d(np.asarray(gamma, np.float64))
    leg_iters = [int(x) for x in leg_iters]
    assert gamma.shape == (len(leg_iters), graph.n) and min(leg_iters) >= 1 and int(stop_after) >= 1
    synd = np.ascontiguousarray(syndromes, np.uint8)
    B, n = synd.shape[0], graph.n
    prior = fu.priors_f64(channel_probs).astype(np.float64)
    mem = np.tile(prior, (B, 1))
    best_w = np.full(B, np.inf)
    nsol = np.zeros(B, np.int64)
    total = np.zeros(B, np.int32)
    first_leg = np.full(B, -1, np.int64)
    replaced = np.zeros(B, np.int64)
    best_dec, best_llr = np.zeros((B, n), np.uint8), np.zeros((B, n), np.float64)
    last_dec, last_llr = np.zeros((B, n), np.uint8), np.zeros((B, n), np.float64)
    active = np.arange(B)
    for leg, (g, iters) in enumerate(zip(gamma, leg_iters)):
        if not len(active):
            break
        a_mem = mu.memory_a(channel_probs, g)
        d, llr, it, cv = memory_leg(graph, prior, a_mem, g, synd[active], None if leg == 0 else mem[active], iters, ms_scaling_factor)
        total[active] += it
        mem[active] = llr
        last_dec[active], last_llr[active] = d, llr
        w = relay_weight(d, prior)
        with np.errstate(invalid="ignore"):
            better = cv & (w < best_w[active])
        rows = active[cv]
        first_leg[rows[nsol[rows] == 0]] = leg
        nsol[rows] += 1
        rows = active[better]
        replaced[rows[nsol[rows] > 1]] += 1  # (nsol counts this solution already)
        best_w[rows] = w[better]
        best_dec[rows], best_llr[rows] = d[better], llr[better]
        active = active[nsol[active] < int(stop_after)]
    conv = nsol > 0
    dec = np.where(conv[:, None], best_dec, last_dec)
    llr = np.where(conv[:, None], best_llr, last_llr)
    out = (dec, llr, total, conv)
    return out + (dict(nsol=nsol, first_leg=first_leg, replaced=replaced, best_w=best_w),) if details else out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
LEG_ITERS = (12, 6, 6, 6, 6, 6)
STOP_AFTER = 3
GAMMA0 = 0.125


def drawn_strengths(n, legs=len(LEG_ITERS), seed=7):
    """Leg 0: 0.125 everywhere; legs 1 .. legs - 1 drawn from [-0.24, 0.66] with a fixed seed."""
    g = np.empty((legs, n), np.float64)
    g[0] = GAMMA0
    g[1:] = np.random.default_rng(seed).uniform(-0.24, 0.66, size=(legs - 1, n))
    return g


@functools.lru_cache(maxsize=None)
def edge_case(code):
    """``mem_bp_util.edge_case`` (its syndromes, max_iter aside) for the relay tests: the first 300 rows, alpha 0.625; surface5 and bb144 with
    non-uniform probabilities p * U[0.5, 1.5] (seed 11) -- with uniform ones equal weights tie and no later solution ever replaces an earlier
    one; hgp_hamming3 keeps its uniform p.  surface5: bp_edge_relay_kernel<1>; bb144: bp_edge8_relay_kernel<9, 3>; hgp_hamming3: <3, 4>."""
    c = dict(mu.edge_case(code))
    n = c["h"].shape[1]
    if code != "hgp_hamming3":
        c["probs"] = c["probs"] * np.random.default_rng(11).uniform(0.5, 1.5, size=n)
    c["synd"] = np.ascontiguousarray(c["synd"][:300])
    c["gamma"] = drawn_strengths(n)
    c["leg_iters"], c["stop_after"] = LEG_ITERS, STOP_AFTER
    del c["max_iter"]
    return c


def first_rows(case, rows):
    c = dict(case)
    c["synd"] = np.ascontiguousarray(case["synd"][:rows])
    return c


_EXPECT: dict = {}


def expected(key, case):
    """The relay restatement's outputs (with details) for a case dict (h, probs, synd, alpha, gamma, leg_iters, stop_after), computed once
    per key and shared read-only."""
    if key not in _EXPECT:
        out = relay_restatement(case["h"], case["probs"], case["gamma"], case["leg_iters"], case["stop_after"], case["synd"], case["alpha"], details=True)
        for x in out[:4]:
            x.setflags(write=False)
        _EXPECT[key] = out
    return _EXPECT[key]


def rows_of(want, rows):
    """The first ``rows`` rows of an expected() result."""
    return tuple(x[:rows] for x in want[:4]) + ({k: v[:rows] for k, v in want[4].items()},)


def shows(want, stop_after):
    """(rows without a solution, rows stopped at stop_after, rows with 1 .. stop_after - 1 solutions, rows first solved after leg 0, rows
    where a later solution replaced an earlier one) of an expected() result."""
    d = want[4]
    return (int(np.count_nonzero(d["nsol"] == 0)), int(np.count_nonzero(d["nsol"] == stop_after)),
            int(np.count_nonzero((d["nsol"] > 0) & (d["nsol"] < stop_after))), int(np.count_nonzero(d["first_leg"] > 0)),
            int(np.count_nonzero(d["replaced"] > 0)))


def assert_shows_something(want, stop_after, what, need_replaced=False):
    """What every GPU comparison asserts on the restatement's own output first -- otherwise it shows nothing."""
    none, stopped, fewer, late, replaced = shows(want, stop_after)
    print(f"{what}: {none} rows without a solution, {stopped} stopped at {stop_after}, {fewer} with fewer, {late} first solved after leg 0, {replaced} replaced")
    assert none > 0, f"{what}: every row finds a solution"
    assert stopped > 0, f"{what}: no row stops at {stop_after} solutions"
    assert fewer > 0, f"{what}: no row ends with fewer than {stop_after} solutions"
    assert late > 0, f"{what}: no row finds its first solution after leg 0"
    if need_replaced:
        assert replaced > 0, f"{what}: no later solution replaces an earlier one"


def ragged_rows(want, stop_after, rows=70, each=3):
    """``rows`` row numbers of an expected() result for the B = 70 batches (64 + 6: a ragged second tile of work): up to ``each`` rows of
    every kind assert_shows_something asks for -- chosen on the RESTATEMENT's output -- then the first rows until there are ``rows``, ascending."""
    d = want[4]
    kinds = (d["nsol"] == 0, d["nsol"] == stop_after, (d["nsol"] > 0) & (d["nsol"] < stop_after), d["first_leg"] > 0, d["replaced"] > 0)
    picked = sorted({int(i) for k in kinds for i in np.flatnonzero(k)[:each]})
    for i in range(len(d["nsol"])):
        if len(picked) >= rows:
            break
        if i not in picked:
            picked.append(i)
    return np.array(sorted(picked[:rows]))


def take(want, idx):
    """The rows ``idx`` of an expected() result."""
    return tuple(x[idx] for x in want[:4]) + ({k: v[idx] for k, v in want[4].items()},)


def masked_strengths(probs, legs, seed=7):
    """drawn_strengths with 0 wherever p is 0 or 1 (their priors are infinite), in every leg."""
    probs = np.asarray(probs, np.float64)
    g = drawn_strengths(len(probs), legs, seed)
    g[:, (probs <= 0.0) | (probs >= 1.0)] = 0.0
    return g
