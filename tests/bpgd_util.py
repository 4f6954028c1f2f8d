"""NumPy restatement of BP with guided decimation, BPGD (``ldpc_hip_bp_set_decimation``) -- the contract the device
reproduces bit for bit -- and the cases the CPU and GPU tests share.

Minimum-sum on the flooding schedule in FP64: the loops of ``f32_util.min_sum_restatement`` at ``np.float64``, with a prior per ROW that a
decimation can change.  ``L0`` is formed as ``upload_priors`` forms it (``f32_util.priors_f64``).  Per syndrome row::

    P = L0; messages = L0 per entry; it = 0
    frozen[j] = not isfinite(L0[j])                  (a column with p = 0, 1 or a NaN prior is never chosen)
    for r = 0 .. R-1:
        repeat up to T times:
            it += 1
            check pass, bit pass and syndrome test exactly as the plain FP64 decode does them, with P in place of L0
                (alpha = 1 - 2^-it with the row's TOTAL it when the scaling factor is 0; a syndrome byte > 1 never converges)
            if the decisions reproduce the syndrome: converge = 1, outputs = this bit pass, iterations = it, STOP
            the backward sums complete the bit-to-check messages
        if r == R-1: break
        M = the posteriors of the last bit pass
        j* = the column with frozen[j] false and M[j] not NaN whose |M[j]| is largest; among equal maxima the SMALLEST j
        if there is one: v = (M[j*] <= 0) ? -C : +C;  P[j*] = v;  every bit-to-check message of column j* = v;  frozen[j*] = true
        (none left: nothing changes, the round still runs)
    converge = 0: outputs = the last bit pass, iterations = R * T

The rows of a batch run side by side; a converged row's outputs are frozen at its convergence iteration and whatever the loop goes on to
compute for it is never read.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

import f32_util as fu


def bpgd_restatement(h, channel_probs, syndromes, round_iters, max_rounds, freeze_llr, ms_scaling_factor, details=False):
    """-> (decoding (B, n) uint8, llr (B, n) float64, iterations (B,) int32, converge (B,) bool); with ``details=True`` a fifth entry, a dict:
    ``frozen`` (B, R - 1) int64 -- the column each row froze after round r, -1 for none (nothing left, or the row had converged) -- and
    ``solved_round`` (B,) int64 -- the round a row converged in, -1: never."""
    T, R, C = int(round_iters), int(max_rounds), np.float64(freeze_llr)
    assert T >= 1 and R >= 1 and T * R < 2 ** 31 and C > 0
    h = sp.csr_matrix(h)
    h.sort_indices()
    m, n = h.shape
    row_ptr, col_idx = h.indptr, h.indices
    nnz = len(col_idx)
    edge_row = np.repeat(np.arange(m), np.diff(row_ptr))
    order = np.lexsort((edge_row, col_idx))  # column by column, rows ascending: CSR edge ids
    col_ptr = np.concatenate(([0], np.cumsum(np.bincount(col_idx, minlength=n)))).astype(np.int64)
    dtype = np.float64
    big = np.float64(np.finfo(dtype).max)
    synd = np.ascontiguousarray(syndromes, np.uint8)
    B = synd.shape[0]
    l0 = fu.priors_f64(channel_probs)
    prior = np.tile(l0, (B, 1))  # P, per row
    frozen = np.tile(~np.isfinite(l0), (B, 1))
    b2c = np.empty((nnz, B), dtype)
    c2b = np.zeros((nnz, B), dtype)
    for e in range(nnz):
        b2c[e] = l0[col_idx[e]]
    dec_out = np.zeros((B, n), np.uint8)
    llr_out = np.zeros((B, n), dtype)
    iters = np.zeros(B, np.int32)
    conv = np.zeros(B, bool)
    dec = np.zeros((B, n), np.uint8)
    llr = np.zeros((B, n), dtype)
    hd = h.toarray().astype(np.int64)
    chosen = np.full((B, max(R - 1, 0)), -1, np.int64)
    solved_round = np.full(B, -1, np.int64)
    rows = np.arange(B)
    it = 0
    with np.errstate(all="ignore"):
        for rnd in range(R):
            for _ in range(T):
                it += 1
                alpha = np.float64(1.0 - 2.0 ** (-it) if ms_scaling_factor == 0.0 else float(ms_scaling_factor))
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
                    temp = prior[:, j].copy()
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
                solved_round[run & ok] = rnd
                conv |= ok
                if conv.all():
                    break
                for j in range(n):
                    temp = np.zeros(B, dtype)
                    for p in range(col_ptr[j + 1] - 1, col_ptr[j] - 1, -1):
                        e = order[p]
                        b2c[e] = b2c[e] + temp
                        temp = temp + c2b[e]
            if conv.all() or rnd == R - 1:
                break
            # ---- decimation: the largest |M| among the columns not frozen and not NaN, the smallest column among equal ones ----
            eligible = ~frozen & ~np.isnan(llr)
            key = np.where(eligible, np.abs(llr), -1.0)
            jstar = key.argmax(axis=1)  # (the first of equal maxima)
            has = eligible[rows, jstar]
            v = np.where(llr[rows, jstar] <= 0, -C, C)
            take = has & ~conv
            chosen[take, rnd] = jstar[take]
            prior[rows[has], jstar[has]] = v[has]
            frozen[rows[has], jstar[has]] = True
            for e in range(nnz):
                hit = has & (jstar == col_idx[e])
                b2c[e][hit] = v[hit]
    out = (dec_out, llr_out, iters, conv)
    return out + (dict(frozen=chosen, solved_round=solved_round),) if details else out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
_EXPECT: dict = {}


def expected(key, case):
    """The restatement's outputs (with details) for a case dict (h, probs, synd, alpha, round_iters, max_rounds, freeze_llr), computed once
    per key and shared read-only."""
    if key not in _EXPECT:
        out = bpgd_restatement(case["h"], case["probs"], case["synd"], case["round_iters"], case["max_rounds"], case["freeze_llr"], case["alpha"], details=True)
        for x in out[:4]:
            x.setflags(write=False)
        _EXPECT[key] = out
    return _EXPECT[key]


def shows(want, max_rounds):
    """(rows solved in round 0, rows solved after at least one decimation, rows that walk every round without a solution) of a result with details."""
    sr, conv = want[4]["solved_round"], want[3]
    return int(np.count_nonzero(sr == 0)), int(np.count_nonzero(sr > 0)), int(np.count_nonzero(~conv))


@functools.lru_cache(maxsize=None)
def tie_case(extra_rounds=2):
    """``rep_code(5)`` with uniform priors, alpha 1, T = 5, C = +inf and a syndrome byte of 2 in every row: no row ever converges, and
    R = n + ``extra_rounds`` walks past "nothing left to freeze".  Rows 0 and 1 (the byte 2 in check 0 / check 3, every parity even): after
    five iterations at alpha 1 every posterior not yet frozen is the same multiple of the prior, so EVERY decimation is a tie among all the
    columns left and they are frozen in ascending order.  Row 2 (a byte 3: odd parity in check 1) has no such symmetry."""
    from ldpc_amd import codes
    h = sp.csr_matrix(codes.rep_code(5))
    synd = np.zeros((3, h.shape[0]), np.uint8)
    synd[0, 0] = 2
    synd[1, 3] = 2
    synd[2, 1] = 3
    return dict(h=h, probs=np.full(h.shape[1], 0.1), synd=synd, alpha=1.0, round_iters=5, max_rounds=h.shape[1] + extra_rounds, freeze_llr=np.inf)


@functools.lru_cache(maxsize=None)
def edge_channel_case(code="hamming3", alpha=0.625, freeze_llr=25.0):
    """``f32_util.small_case`` -- its channel has p = 0, 1, 0.5 and 1e-300 -- as a BPGD case: T = 2, R = n + 1."""
    c = fu.small_case(code, alpha)
    return dict(h=c["h"], probs=c["probs"], synd=c["synd"], alpha=alpha, round_iters=2, max_rounds=c["h"].shape[1] + 1, freeze_llr=freeze_llr)
