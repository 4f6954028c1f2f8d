"""Shared by tests/test_row_priors_edge_cases.py (CPU) and tests/test_gpu_row_priors_edge.py (GPU): row-prior batches for the codes of the lane = edge
families (bp_edge_rp_kernel<R>, bp_edge8_rp_kernel<R, DC>: ldpc_amd/csrc/bp_edge_rp_kernel.h), and what the per-row oracle --
``oracle.BpOracle(h, error_channel=P[b], ...).decode_batch(S[b:b+1])``, the CPU restatement of the reference's ``update_channel_probs(P[b]);
decode(S[b])`` loop -- returns for them.  Everything is built once and shared (treat as read-only).

The codes, their 131 syndromes and the handle's own per-column probabilities are those of tests/ladder_util.py: for every R of plan_edge and
every (R, DC) of plan_edge8 the smallest per-column ("percol") case.  The row probabilities come from tests/row_priors_util.py: ordinary
levels around p = 0.08, different in every row, and the special values (p = 0, 1, 0.5, 1e-300, 1 - 2^-53) over a third of the bits of rows in
both full tiles of 64 and in the 3-row tail."""
import functools
import os

import numpy as np
import scipy.sparse as sp

import ladder_util as lu
import row_priors_util
from row_priors_util import SPECIAL, draw_levels, levels_around

# The reference's fixtures for these codes (tests/golden/make_golden_row_priors_edge.py), in the format of tests/golden/row_priors/ but in a
# directory of their own: tests/test_row_priors_api.py pins the list of files there name by name.
EDGE_FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_priors_edge")
EDGE_FIXTURES = ("row_priors_bb144_ms10_osd0", "row_priors_surface_ms_adaptive")


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    """``row_priors_util.load_case`` for either directory (its loader reads the directory's name when it is called); arrays read-only."""
    saved = row_priors_util.ROW_PRIORS_DIR
    try:
        if name in EDGE_FIXTURES:
            row_priors_util.ROW_PRIORS_DIR = EDGE_FIXTURE_DIR
        c = row_priors_util.load_case(name)
    finally:
        row_priors_util.ROW_PRIORS_DIR = saved
    for k in ("probs", "syndromes", "decoding", "converge", "iterations", "llr", "llr_crc"):
        c[k].setflags(write=False)
    return c


SPECIAL_ROWS = (3, 40, 70, 100, 129, 130)  # tiles 0, 0, 1, 1 and the tail 128 .. 130
RP_KERNELS = ("bp_edge_rp_kernel", "bp_edge8_rp_kernel")
POOL_ROWS = 20011


def rp_kernel_name(plain):
    """'bp_edge_kernel<3, false, false>' -> 'bp_edge_rp_kernel<3>'; 'bp_edge8_kernel<4, 3, false>' -> 'bp_edge8_rp_kernel<4, 3>'."""
    base, args = plain.rstrip(">").split("<")
    args = [a.strip() for a in args.split(",")]
    if base == "bp_edge_kernel":
        return f"bp_edge_rp_kernel<{args[0]}>"
    assert base == "bp_edge8_kernel", plain
    return f"bp_edge8_rp_kernel<{args[0]}, {args[1]}>"


def _smallest_percol():
    """One case per instantiation: of the per-column cases that name it, the one with the fewest rows."""
    best = {}
    for c in lu.EDGE_CASES + lu.EDGE8_CASES:
        if c.uniform:
            continue
        if c.kernel not in best or c.build["m"] < best[c.kernel].build["m"]:
            best[c.kernel] = c
    return list(best.values())


CASES = _smallest_percol()
CASE_BY_ID = {c.id: c for c in CASES}


def draw_rows(seed, shape, levels, special_rows):
    """``draw_levels`` (which asserts that no two rows drew the same priors); a code of a handful of bits can draw a row twice, and then
    the next seed is taken."""
    for k in range(64):
        try:
            return draw_levels(np.random.default_rng(seed + 7919 * k), shape, levels, special_rows=special_rows)
        except AssertionError:
            continue
    raise AssertionError(f"no seed gives {shape[0]} different rows of {shape[1]} priors")


@functools.lru_cache(maxsize=None)
def row_probs(case_id, special=True):
    """P (131, n) of a ladder case (percol, uniform or outside)."""
    c = next(c for c in lu.ALL_CASES if c.id == case_id)
    h, _, synd = lu.inputs(case_id)
    levels = levels_around(0.08, count=11, spread=4.0)
    idx = draw_rows(c.seed + 17, (len(synd), h.shape[1]), levels, SPECIAL_ROWS if special else ())
    probs = np.ascontiguousarray(levels[idx], np.float64)
    probs.setflags(write=False)
    return probs


def per_row_oracle(h, probs, synd, max_iter, method, alpha):
    import oracle
    dec = np.zeros((len(synd), h.shape[1]), np.uint8)
    llr = np.zeros((len(synd), h.shape[1]), np.float64)
    it = np.zeros(len(synd), np.int32)
    cv = np.zeros(len(synd), bool)
    with np.errstate(all="ignore"):
        for b in range(len(synd)):
            d, l, i, c = oracle.BpOracle(h, error_channel=probs[b], max_iter=max_iter, bp_method=method, ms_scaling_factor=alpha).decode_batch(synd[b:b + 1])
            dec[b], llr[b], it[b], cv[b] = d[0], l[0], i[0], c[0]
    for x in (dec, llr, it, cv):
        x.setflags(write=False)
    return dec, llr, it, cv


@functools.lru_cache(maxsize=None)
def expected(case_id, method=None, special=True):
    """The per-row oracle's (decoding, llr, iterations, converge) of a ladder case decoded with ``row_probs(case_id, special)``."""
    c = next(c for c in lu.ALL_CASES if c.id == case_id)
    h, _, synd = lu.inputs(case_id)
    return per_row_oracle(h, row_probs(case_id, special), synd, lu.MAX_ITER, method or c.method, c.alpha)


# ---- BB [[144,12,12]]: the work-pool batch and the routing checks --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bb144():
    """(h, own probabilities, syndromes (70, m), P (70, n) without special values, max_iter, alpha): tests/f32_util.py's BB144 case with
    row priors at levels around its p = 0.06."""
    import f32_util as fu
    c = fu.bb144_case()
    h = sp.csr_matrix(c["h"])
    levels = levels_around(0.06, count=11, spread=2.0)
    idx = draw_rows(4404, (len(c["synd"]), h.shape[1]), levels, ())
    probs = np.ascontiguousarray(levels[idx], np.float64)
    probs.setflags(write=False)
    return h, np.asarray(c["probs"]), np.asarray(c["synd"]), probs, c["max_iter"], c["alpha"]


@functools.lru_cache(maxsize=None)
def bb144_expected():
    h, _, synd, probs, max_iter, alpha = bb144()
    return per_row_oracle(h, probs, synd, max_iter, "minimum_sum", alpha)


POOL_CASES = {"edge-R1": "edge-R1-m16-percol", "bb144": None}


def pool_inputs(key):
    """-> (h, own probs, S (70 | 131, m), P, max_iter, alpha, expected, kernel) of a work-pool case; rows are drawn from it by index."""
    if POOL_CASES[key] is None:
        h, own, synd, probs, max_iter, alpha = bb144()
        return h, own, synd, probs, max_iter, alpha, bb144_expected(), "bp_edge8_rp_kernel<9, 3>"
    cid = POOL_CASES[key]
    c = next(c for c in lu.ALL_CASES if c.id == cid)
    h, own, synd = lu.inputs(cid)
    return h, own, synd, row_probs(cid, special=False), lu.MAX_ITER, c.alpha, expected(cid, special=False), rp_kernel_name(c.kernel)


def pool_index(rows):
    return (np.arange(POOL_ROWS, dtype=np.int64) * 37) % rows


def distinct_rows(probs):
    """Rows of ``probs`` whose priors differ from every other row's."""
    keys = [row.tobytes() for row in np.ascontiguousarray(probs)]
    count = {}
    for k in keys:
        count[k] = count.get(k, 0) + 1
    return np.array([count[k] == 1 for k in keys])


def has_special(probs):
    """Per row: does it hold one of the special probabilities?"""
    return np.isin(probs, np.array(SPECIAL)).any(axis=1)
