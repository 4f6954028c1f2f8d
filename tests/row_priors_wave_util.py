"""Shared by tests/test_row_priors_wave_cases.py (CPU) and tests/test_gpu_row_priors_wave.py (GPU): row-prior batches for the codes of the
lane = node kernel (bp_wave_rp_kernel<DR, DC, TEAM>: ldpc_amd/csrc/bp_wave_rp_kernel.h), and what the per-row oracle --
``oracle.BpOracle(h, error_channel=P[b], ...).decode_batch(S[b:b+1])``, the CPU restatement of the reference's ``update_channel_probs(P[b]);
decode(S[b])`` loop -- returns for them.  Everything is built once and shared (treat as read-only).

The codes are the eight of tests/relay_wave_util.py -- just outside both lane = edge ladders, one or two per rung of (4,2) (4,4) (6,3) (8,4)
(8,8) (16,8), each small enough for one slot of the slot kernel -- and ``hgp1600``, the [[1600,64]] hypergraph product, whose slot does not fit
150 KiB: the code that went to the per-pass kernels before this kernel.  Per case: B = 131 rows, probabilities at eleven levels around the
case's p (p / 4 .. 4 p), different in every row, the special values (p = 0, 1, 0.5, 1e-300, 1 - 2^-53) over a third of the bits of
``SPECIAL_ROWS``; syndromes of errors drawn at each row's own rates; row 0 all zero, a syndrome byte 2 in row 7 and a byte 3 in row 90;
alpha 0.625 (and, once per rung, alpha 0: the adaptive factor), 20 iterations.  Nothing here imports the library's dispatch: its size
rules are written out again."""
import functools
import os

import numpy as np
import scipy.sparse as sp

import relay_wave_util as wu
import row_priors_edge_util as eu
import row_priors_util
from row_priors_util import SPECIAL, levels_around, syndromes_of

WAVE_FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_priors_wave")
WAVE_FIXTURES = ("row_priors_hgp400_ms12_osd0", "row_priors_ldpc128_ms_adaptive")
# the min-sum fixtures of the other two directories, with the rung their code lands on
OLDER_FIXTURES = {"row_priors_hamming3_ms": (4, 4), "row_priors_rep5_ms": (4, 2), "row_priors_bb144_ms10_osd0": (6, 3), "row_priors_surface_ms_adaptive": (4, 2)}
FIXTURE_RUNG = {"row_priors_hgp400_ms12_osd0": (8, 4), "row_priors_ldpc128_ms_adaptive": (16, 8), **OLDER_FIXTURES}

BATCH = 131
MAX_ITER = 20
ALPHA = 0.625
SPECIAL_ROWS = (3, 40, 70, 100, 129, 130)  # on both sides of rows 64 and 128
ZERO_ROW, BYTE2_ROW, BYTE3_ROW = 0, 7, 90
POOL_ROWS = eu.POOL_ROWS
POOL_CASES = ("ldpc64_58", "surface23")
RP_KERNEL = "bp_wave_rp_kernel"


def _hgp1600():
    from ldpc_amd.codes.synthetic import hypergraph_product_hx, regular_ldpc_code
    return hypergraph_product_hx(regular_ldpc_code(n=32, dv=3, dc=4, seed=5))


# name -> (rung, p, seed of the draw).  (A draw that misses a condition of tests/test_row_priors_wave_cases.py gets another seed, never another condition.)
CASES = {name: (rung, p, 9100 + 10 * k) for k, (name, (rung, _, p)) in enumerate(wu.CASES.items())}
CASES["surface23"] = ((4, 2), 0.03, 9121)  # (seed 9100 left 6 rows that converge before max_iter: d = 23 at these rates mostly runs to the end)
CASES["hgp1600"] = ((8, 4), 0.02, 9190)
SLOT_CASES = tuple(wu.CASES)           # fit one slot of the slot kernel
ADAPTIVE = {"surface23": (4, 2), "ldpc132_34": (4, 4), "bb288": (6, 3), "hgp400": (8, 4), "ldpc64_58": (8, 8), "ldpc128_516": (16, 8)}  # alpha 0, once per rung


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name in wu.CASES:
        return wu.matrix(name)
    h = sp.csr_matrix(_hgp1600(), dtype=np.uint8)
    h.eliminate_zeros()
    h.sort_indices()
    return h


def kernel_name(rung, team):
    return f"{RP_KERNEL}<{rung[0]}, {rung[1]}, {'true' if team else 'false'}>"


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(h, own, probs (131, n), synd (131, m), rung): the handle's own probabilities are the case's p on every bit."""
    rung, p, seed = CASES[name]
    h = matrix(name)
    m, n = h.shape
    levels = levels_around(p, count=11, spread=4.0)
    idx = eu.draw_rows(seed, (BATCH, n), levels, SPECIAL_ROWS)
    probs = np.ascontiguousarray(levels[idx], np.float64)
    synd = syndromes_of(h, np.clip(probs, 0.0, 0.5), np.random.default_rng(seed + 1))
    synd[ZERO_ROW] = 0
    synd[BYTE2_ROW, 0] = 2   # a byte > 1: never converges (bp.hpp:300)
    synd[BYTE3_ROW, m - 1] = 3
    for x in (probs, synd):
        x.setflags(write=False)
    return dict(h=h, own=np.full(n, p), probs=probs, synd=synd, rung=rung)


@functools.lru_cache(maxsize=None)
def expected(name, alpha=ALPHA):
    """The per-row oracle's (decoding, llr, iterations, converge) of a case."""
    c = case(name)
    return eu.per_row_oracle(c["h"], c["probs"], c["synd"], MAX_ITER, "minimum_sum", alpha)


@functools.lru_cache(maxsize=None)
def expected_product_sum(name):
    c = case(name)
    return eu.per_row_oracle(c["h"], c["probs"], c["synd"], MAX_ITER, "product_sum", 1.0)


def pool_index(rows):
    return eu.pool_index(rows)


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    """``row_priors_util.load_case`` for any of the three directories (its loader reads the directory's name when it is called); arrays read-only."""
    if name not in WAVE_FIXTURES:
        return eu.load_fixture(name)
    saved = row_priors_util.ROW_PRIORS_DIR
    try:
        row_priors_util.ROW_PRIORS_DIR = WAVE_FIXTURE_DIR
        c = row_priors_util.load_case(name)
    finally:
        row_priors_util.ROW_PRIORS_DIR = saved
    for k in ("probs", "syndromes", "decoding", "converge", "iterations", "llr", "llr_crc"):
        c[k].setflags(write=False)
    return c


def special_kinds(probs):
    """The special probabilities that occur in ``probs``."""
    return {v for v in SPECIAL if (probs == v).any()}


# ---- the dispatch's size rules, restated (host_onchip.h: small_lds_bytes; bp_small_kernel.h: small_slot_bytes; plan_wave_rp) ----------------
def small_slot_bytes(h, rp=True):
    m, n = h.shape
    return ((h.nnz * 16 + n * 8 + n + m + 15) & ~15) + (n * 8 if rp else 0)


def small_lds_bytes(h, slots=1, rp=True):
    """LDS of the slot kernel for ``slots`` resident syndromes: the log table, the priors, the CSR and CSC tables, then the slots."""
    m, n = h.shape
    fixed = 256 * 8 + n * 8 + (m + 1 + h.nnz + n + 1 + h.nnz) * 4
    return ((fixed + 15) & ~15) + small_slot_bytes(h, rp) * slots


SLOT_BUDGET = 150 * 1024


def wave_rp_lds_bytes(h):
    """LDS of one syndrome on its rung (bp_wave_rp_kernel.h: wave_rp_lds_shared / _private -- the relay kernel's sizes)."""
    return wu.wave_lds_bytes(h)
