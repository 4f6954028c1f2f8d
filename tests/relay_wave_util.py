"""The cases of the lane = node Relay-BP / memory kernel (bp_wave_relay_kernel), shared by the CPU test of the cases
(tests/test_relay_wave_cases.py) and the GPU tests (tests/test_gpu_relay_wave.py), and the size rules of the dispatch restated.

Each case is a real code just outside both lane = edge ladders, one per rung of the ladder of bp_wave_relay_kernel -- (4,2) (4,4) (6,3) (8,4)
(8,8) (16,8) -- with channel probabilities p * U[0.5, 1.5] (seed 1), 300 syndromes of errors drawn with them (seed 2), alpha 0.625 and
``relay_bp_util.masked_strengths``.  ``legs=4``: legs of (8, 4, 4, 4) iterations, stop after 2 solutions; ``legs=6``: (12, 6, 6, 6, 6, 6), stop
after 3 -- the schedule on which a later, lighter solution replaces an earlier one often enough to be asserted.  Nothing here imports the
library's dispatch: the rules are written out again, as ladder_util.py does."""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

import relay_bp_util as ru

ALPHA = 0.625
SCHEDULES = {4: ((8, 4, 4, 4), 2), 6: ((12, 6, 6, 6, 6, 6), 3)}
RUNGS = ((4, 2), (4, 4), (6, 3), (8, 4), (8, 8), (16, 8))


def _bb288():
    from ldpc_amd.codes.synthetic import bivariate_bicycle_hx
    return bivariate_bicycle_hx(12, 12, (("x", 3), ("y", 2), ("y", 7)), (("y", 3), ("x", 1), ("x", 2)))


def _hgp400():
    from ldpc_amd.codes.synthetic import hypergraph_product_hx, regular_ldpc_code
    return hypergraph_product_hx(regular_ldpc_code(16, 3, 4, seed=5))


def _bb144x3():
    from test_dem_sampler_twin import dem_models
    return dem_models()["bb144x3"][0]


def _surface23():
    from ldpc_amd.codes.synthetic import rotated_surface_code_x
    return rotated_surface_code_x(23)


def _ldpc(n, dv, dc):
    from ldpc_amd.codes.synthetic import regular_ldpc_code
    return lambda: regular_ldpc_code(n, dv, dc, seed=3)


# name -> (rung, builder, p)
CASES = {
    "surface23": ((4, 2), _surface23, 0.03),               # 264 x 529
    "ldpc132_34": ((4, 4), _ldpc(132, 3, 4), 0.07),        # 99 x 132
    "ldpc200_36": ((6, 3), _ldpc(200, 3, 6), 0.05),        # 100 x 200
    "bb288": ((6, 3), _bb288, 0.05),                       # 144 x 288
    "hgp400": ((8, 4), _hgp400, 0.04),                     # 192 x 400
    "bb144x3": ((8, 4), _bb144x3, 0.02),                   # 216 x 576
    "ldpc64_58": ((8, 8), _ldpc(64, 5, 8), 0.06),          # 40 x 64
    "ldpc128_516": ((16, 8), _ldpc(128, 5, 16), 0.02),     # 40 x 128
}
SIX_LEGS = ("surface23", "bb288", "hgp400", "bb144x3")    # the cases that are also decoded with the six-leg schedule


@functools.lru_cache(maxsize=None)
def matrix(name):
    h = sp.csr_matrix(CASES[name][1](), dtype=np.uint8)
    h.eliminate_zeros()
    h.sort_indices()
    return h


@functools.lru_cache(maxsize=None)
def case(name, legs=4):
    h = matrix(name)
    n = h.shape[1]
    p = CASES[name][2]
    probs = p * np.random.default_rng(1).uniform(0.5, 1.5, size=n)
    errors = (np.random.default_rng(2).random((300, n)) < probs).astype(np.uint8)
    synd = np.ascontiguousarray((errors @ h.T.toarray().astype(np.uint8)) & 1, np.uint8)
    leg_iters, stop = SCHEDULES[legs]
    return dict(h=h, probs=probs, synd=synd, alpha=ALPHA, gamma=ru.masked_strengths(probs, len(leg_iters)), leg_iters=leg_iters, stop_after=stop)


def want(name, legs=4):
    return ru.expected(f"wave|{name}|{legs}", case(name, legs))


def batch70(name, legs=4):
    """(case, expected) of the B = 70 batch picked from the 300 rows on the restatement's output (relay_bp_util.ragged_rows)."""
    full, w = case(name, legs), want(name, legs)
    idx = ru.ragged_rows(w, full["stop_after"], 70)
    return dict(full, synd=np.ascontiguousarray(full["synd"][idx])), ru.take(w, idx)


def tiled(name, rows, legs=4):
    """(case, expected) of ``rows`` rows: the 300 rows of the case repeated."""
    full, w = case(name, legs), want(name, legs)
    idx = np.arange(rows) % 300
    return dict(full, synd=np.ascontiguousarray(full["synd"][idx])), ru.take(w, idx)


# ---- the dispatch's size rules, restated (host_onchip.h: plan_edge, plan_edge8, pick_wave / plan_wave_relay) ----------------------------------
def degrees(h):
    h = sp.csr_matrix(h)
    return int(np.diff(h.indptr).max()), int(np.bincount(h.indices, minlength=h.shape[1]).max())


def edge_takes(h):
    """plan_edge: rows <= 4, columns <= 2, 4 m slots in at most 16 rounds of 64."""
    dr, dc = degrees(h)
    return dr <= 4 and dc <= 2 and (4 * h.shape[0] + 63) // 64 <= 16


def edge8_takes(h):
    """plan_edge8: rows <= 8, columns <= 4, 8 m slots in at most 12 rounds (columns <= 3) or 9 rounds (columns of 4)."""
    dr, dc = degrees(h)
    return dr <= 8 and dc <= 4 and (8 * h.shape[0] + 63) // 64 <= (12 if dc <= 3 else 9)


def wave_rung(h):
    """The (DR, DC) instantiation the code lands on, or None (rows > 16 or columns > 8)."""
    dr, dc = degrees(h)
    for r, c in RUNGS:
        if dr <= r and dc <= c:
            return r, c
    return None


def wave_lds_bytes(h):
    """LDS of one syndrome on its rung: the shared tables + the private region (bp_wave_relay_kernel.h: wave_relay_lds_shared / _private)."""
    r, c = wave_rung(h)
    m, n = h.shape
    mp, np_ = (m + 63) // 64 * 64, (n + 63) // 64 * 64
    up16 = lambda b: (b + 15) & ~15  # noqa: E731
    return up16(r * mp * 2 + c * np_ * 2 + mp) + up16((r * mp + 2) * 8 + np_ * 8 + (np_ // 64 + 1) * 8 + mp)


def padded_tables(a, gamma, np_):
    """wave_relay_table_kernel in NumPy: a and gamma (legs, n) padded to np_ columns with a = 1.0 and gamma = 0."""
    a, gamma = np.atleast_2d(a), np.atleast_2d(gamma)
    legs, n = a.shape
    ap, gp = np.ones((legs, np_), np.float64), np.zeros((legs, np_), np.float64)
    ap[:, :n], gp[:, :n] = a, gamma
    return ap, gp
