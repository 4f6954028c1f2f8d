"""The cases of guided decimation on the lane = node kernel (bp_wave_gd_kernel), shared by the CPU test of the cases
(tests/test_bpgd_wave_cases.py) and the GPU tests (tests/test_gpu_bpgd_wave.py).  The contract is tests/bpgd_util.py's restatement, which is
tied to no kernel family; the codes are those of tests/relay_wave_util.py -- one per rung of the kernel's ladder, each just outside both
lane = edge ladders -- with that file's per-column priors and syndromes.  A case is a dict (h, probs, synd, alpha, round_iters, max_rounds,
freeze_llr), as bpgd_util.expected takes it."""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

import bpgd_util as gu
import f32_util as fu
import relay_wave_util as wu

ALPHA = 0.625
T, R, C = 3, 6, 25.0

# (rows solved in round 0, rows solved after a decimation, rows never solved) of every_instantiation(name), measured on the restatement
SHOWS = {"surface23": (11, 4, 55), "ldpc132_34": (42, 26, 2), "ldpc200_36": (24, 36, 10), "bb288": (17, 47, 6), "hgp400": (14, 34, 22),
         "bb144x3": (42, 25, 3), "ldpc64_58": (34, 24, 12), "ldpc128_516": (36, 22, 12)}


def _case(h, probs, synd, alpha=ALPHA, round_iters=T, max_rounds=R, freeze_llr=C):
    return dict(h=h, probs=probs, synd=np.ascontiguousarray(synd, np.uint8), alpha=alpha, round_iters=round_iters, max_rounds=max_rounds, freeze_llr=freeze_llr)


def take(want, idx):
    """Rows ``idx`` of a restatement result with details."""
    return tuple(x[idx] for x in want[:4]) + ({k: v[idx] for k, v in want[4].items()},)


# ---- 1. every instantiation: the first 70 rows of each relay_wave_util case ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def every_instantiation(name):
    c = wu.case(name)
    return _case(c["h"], c["probs"], c["synd"][:70])


def want_instantiation(name):
    return gu.expected(f"wave_gd|{name}|70", every_instantiation(name))


# ---- 2. all 300 rows of a case (the work pool's tiles, B = 300) -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_rows(name):
    c = wu.case(name)
    return _case(c["h"], c["probs"], c["synd"])


def want_all_rows(name):
    return gu.expected(f"wave_gd|{name}|300", all_rows(name))


POOL_ROWS = 20011  # (above the 256 x 16 wavefronts and the 2 048 teams resident at once: every one decodes several syndromes)


def tiled(name, rows):
    """(case, expected) of ``rows`` rows: the 300 rows of the case repeated (relay_wave_util.tiled's indexing)."""
    full, w = all_rows(name), want_all_rows(name)
    idx = np.arange(rows) % 300
    return dict(full, synd=np.ascontiguousarray(full["synd"][idx])), take(w, idx)


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_case():
    """``rep_code(258)``: 257 x 258, rows of 2 and columns of at most 2 but 257 checks -- outside both lane = edge ladders, rung (4,2).
    Uniform p = 0.1, alpha 1, T = 2, R = 6, C = +inf; a syndrome byte 2 at check 0, a byte 2 at check 100, a byte 3 at check 5: no row
    converges, and after two iterations at alpha 1 whole runs of columns hold the same posterior."""
    from ldpc_amd import codes
    h = sp.csr_matrix(codes.rep_code(258))
    synd = np.zeros((3, h.shape[0]), np.uint8)
    synd[0, 0], synd[1, 100], synd[2, 5] = 2, 2, 3
    return _case(h, np.full(h.shape[1], 0.1), synd, alpha=1.0, round_iters=2, max_rounds=6, freeze_llr=np.inf)


# ---- 4. nothing left to freeze ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_frozen_case():
    """ldpc64_58, its first 3 syndromes with byte 0 set to 2 (no row converges), T = 1, R = 67: 64 columns to freeze, then none for two rounds."""
    c = wu.case("ldpc64_58")
    synd = c["synd"][:3].copy()
    synd[:, 0] = 2
    return _case(c["h"], c["probs"], synd, round_iters=1, max_rounds=67)


# ---- 5. special priors ---------------------------------------------------------------------------------------------------------------------------
SPECIAL_COLUMNS = {0: 0.0, 1: 1.0, 2: 0.5, 3: 1e-300, 17: 1.0, 40: 0.0, 41: 0.5, 63: 1e-300}
SPECIAL = [(0.625, 25.0), (1.25, 25.0), (0.625, np.inf), (1.25, np.inf)]  # (alpha, C)


@functools.lru_cache(maxsize=None)
def special_priors_case(alpha, freeze_llr):
    """ldpc64_58 with columns at p = 0, 1, 0.5 and 1e-300 (priors +inf, -inf, +0.0, 690.8); 70 syndromes of errors drawn from that channel
    (seed 5); T = 2, R = 8."""
    base = wu.case("ldpc64_58")
    h = base["h"]
    probs = base["probs"].copy()
    probs[list(SPECIAL_COLUMNS)] = list(SPECIAL_COLUMNS.values())
    errors = (np.random.default_rng(5).random((70, h.shape[1])) < probs).astype(np.uint8)
    return _case(h, probs, (errors @ h.T.toarray().astype(np.uint8)) & 1, alpha=alpha, round_iters=2, max_rounds=8, freeze_llr=freeze_llr)


# ---- 6. an empty column ------------------------------------------------------------------------------------------------------------------------
EMPTY_COLUMN_RATE = 0.02  # (33 of the 70 rows solved in round 0, 37 decimate five times; at 0.05 it is 14 and 56, at 0.12 none and 70)


@functools.lru_cache(maxsize=None)
def empty_column_case():
    """ladder_util's ``outside-empty-column`` (40 checks, a column without entries: no lane = edge family takes it) with its per-column priors
    and 70 syndromes of BSC errors at EMPTY_COLUMN_RATE (seed 77)."""
    import ladder_util as lu
    h, probs, _ = lu.inputs("outside-empty-column")
    return _case(sp.csr_matrix(h), np.array(probs), fu.bsc_syndromes(h, 70, EMPTY_COLUMN_RATE, 77))


# ---- 7. one round is the plain decode -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_round_case():
    c = wu.case("bb288")
    return _case(c["h"], c["probs"], c["synd"][:70], round_iters=12, max_rounds=1)
