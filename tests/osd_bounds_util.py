"""Shared by tests/test_osd_bounds_cases.py (CPU) and tests/test_gpu_osd_bounds.py (GPU): parity-check matrices of EXACTLY the stated shape and
rank, and a case table that stands on every bound at which the OSD code changes its path -- the rungs of osd0_reg_kernel / osdw_reg_kernel (full and
one step past), k = n - rank H around 0, 32, 64 and 128 (osdw_reg_kernel's T records and kwords), the bounds of osd0_flat_kernel, and the heights at
which osd_big_kernel picks another osd_block_eliminate<MQ> (device functions: the launch log cannot see them, only a matrix of that height runs them).

(What the k cases can and cannot see in osdw_reg_kernel: a 32-column group of T left unwritten changes decisions at k = 1 and k = 65; the clear of the
upper half of the last T word does not -- every candidate mask and every single-column lane stops at bit k, so no result reads those bits.)

expected_kernel restates the choice of plan_osd / plan_osd_big (ldpc_amd/csrc/host_osd.h) and the LDS sizes of csrc/osd_kernels.h it depends on; nothing is
imported from the library.

Inputs of every case: min-sum BP (scaling 0.8) for a few iterations at a high error rate with non-uniform priors, so that most rows reach OSD and few
candidate weights tie; rank-deficient cases (dup > 0, or more rows than columns) get every fifth syndrome pushed outside the image of H (status 2,
osd_exact_kernel, the second pass through the same kernel)."""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

ALPHA = 0.8


def bounds_code(m, n, seed, row_extra=3, dup=0, heavy=0):
    """A seeded m x n matrix of exactly known rank, and the rows that are copies.  The core is [T | A] with r = min(m, n) rows: T unit lower
    triangular r x r with up to two further entries per row, A r x (n - r) with row_extra entries per row (fewer where A is narrower); rows and
    columns are then permuted.  m > n: the m - n further rows are copies of core rows.  `dup` core rows are overwritten by copies of others.  So
    rank = min(m, n) - dup, k = n - rank, and every row has at most 3 + row_extra entries -- except one row raised to exactly `heavy` entries.
    Returns (csr matrix, [(copy, original), ...])."""
    rng = np.random.default_rng(seed)
    r = min(m, n)
    assert 0 <= dup < r
    core = np.zeros((r, n), np.uint8)
    for i in range(r):
        core[i, i] = 1
        if i:
            core[i, rng.choice(i, size=min(i, int(rng.integers(0, 3))), replace=False)] = 1
        if n > r:
            core[i, r + rng.choice(n - r, size=min(row_extra, n - r), replace=False)] = 1
    if heavy:
        i = int(rng.integers(r // 2, r))
        free = r + np.flatnonzero(core[i, r:] == 0)
        core[i, rng.choice(free, size=heavy - int(core[i].sum()), replace=False)] = 1
    core = core[rng.permutation(r)][:, rng.permutation(n)]
    assert 2 * dup <= r, "dup is at most half the core rows"
    rows = rng.choice(r, size=2 * dup, replace=False)
    copies = [(int(dst), int(src)) for dst, src in zip(rows[:dup], rows[dup:])]
    for dst, src in copies:
        core[dst] = core[src]
    copies += [(r + i, int(src)) for i, src in enumerate(rng.integers(0, r, size=m - r))]
    h = np.concatenate([core, core[[src for _, src in copies[dup:]]]]) if m > r else core
    return sp.csr_matrix(h), copies


def gf2_rank(h):
    """Rank over GF(2) by a dense elimination on bit-packed rows."""
    a = np.packbits(np.asarray(h.toarray() if sp.issparse(h) else h, np.uint8), axis=1)
    rank = 0
    for c in range(a.shape[1] * 8):
        if rank == a.shape[0]:
            break
        byte, bit = c >> 3, 0x80 >> (c & 7)
        hit = np.flatnonzero(a[rank:, byte] & bit)
        if not len(hit):
            continue
        p = rank + int(hit[0])
        a[[rank, p]] = a[[p, rank]]
        rows = np.flatnonzero(a[:, byte] & bit)
        rows = rows[rows != rank]
        a[rows] ^= a[rank]
        rank += 1
    return rank


# ---- which kernel: plan_osd / plan_osd_big restated ----------------------------------------------------------------------------------------
REG_RUNGS = ((64, 2, 1), (128, 3, 2), (128, 4, 2), (256, 8, 4))  # (m <=, 64-bit words of [H | s] <=, R): osd0_reg_kernel<R, W> / osdw_reg_kernel<R, W>
FLAT_DWORDS = (2, 3, 5, 8)  # osd0_flat_kernel<R, D>: n <= 32 D
BLOCK_ROWS = 2048           # osd_block_eliminate: up to eight rows per thread
LDS_ROOM = 150 * 1024


def _align(x, a):
    return (x + a - 1) & ~(a - 1)


def one_wave_lds(m, n, words, higher):
    """osd_lds_layout: per-wavefront LDS of osd0_kernel / osdw_kernel."""
    t = m * words * 8
    keys = t + (m * 8 if higher else 0)
    order = keys + n * 8
    code = order + n * 4
    npcol = code + n * 4
    pivot_col = npcol + n * 4 if higher else code
    x = pivot_col + m * 4
    return _align(x + (0 if higher else n), 16)


def big_lds(m, n, higher, blocked, nplanes):
    """osd_big_lds_bytes: the workgroup kernel's LDS without the working copy of H."""
    hwords = (n + 63) // 64
    pow2 = 1
    while pow2 < n:
        pow2 <<= 1
    room = _align(_align(m * 5 + 1, 8) + pow2 * 2, 16)
    sort = room + n * 8
    elim = room + m * 8 + (16 * 9 * 16 * 8 if blocked else 0)
    weigh = _align(room + 2 * n, 8) + (7 * hwords + (m + 1) * nplanes) * 8 if higher else 0
    return _align(max(sort, elim, weigh), 16)


def expected_kernel(m, n, max_row_deg, higher, osd_kernel_mode, no_flat=False, unblocked=False):
    """The instantiation an OSD call launches, as the launch log spells it.  higher: OSD_E / OSD_CS at an order > 0; osd_kernel_mode: what
    set_osd_kernel was given (-1 automatic, 0 the one-wavefront LDS kernels while they fit, 2 osd_big_kernel with H in a global slot)."""
    words = (n + 1 + 63) // 64
    reg, force_big = osd_kernel_mode != 0, osd_kernel_mode == 2
    rung = None if not reg or force_big else next(((r, w) for mm, w, r in REG_RUNGS if m <= mm and words <= w), None)
    if rung and higher:
        return f"osdw_reg_kernel<{rung[0]}, {rung[1]}>"
    if rung:
        if m <= 128 and n <= 256 and max_row_deg <= 8 and not no_flat:
            return f"osd0_flat_kernel<{1 if m <= 64 else 2}, {next(d for d in FLAT_DWORDS if 32 * d >= n)}>"
        return f"osd0_reg_kernel<{rung[0]}, {rung[1]}>"
    per_wave = one_wave_lds(m, n, words, higher)
    if not (per_wave > LDS_ROOM or force_big or (reg and per_wave > 40 * 1024)):
        return "osdw_kernel" if higher else "osd0_kernel"
    blocked = m <= BLOCK_ROWS and not unblocked
    mat_bytes = (n + 63) // 64 * m * 8
    # (how many wavefronts weigh candidates -- 4, 2 or 1 staged planes -- follows the batch; a case whose MAT_LDS would depend on it has no one answer)
    fits = {big_lds(m, n, higher, blocked, nb) + mat_bytes <= LDS_ROOM for nb in ((4, 2, 1) if higher else (0,))}
    assert len(fits) == 1, f"{m} x {n}: whether H fits LDS depends on the number of staged planes"
    return f"osd_big_kernel<{_b(higher)}, {_b(not force_big and fits.pop())}>"


def block_rows_per_thread(m):
    """osd_big_kernel: the MQ of osd_block_eliminate<MQ> a matrix of m rows runs (0: the one-pivot-per-step loop)."""
    return next((q for q in (1, 2, 3, 4, 6, 8) if m <= 256 * q), 0)


def _b(x):
    return "true" if x else "false"


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
OSD0, OSD_E, OSD_CS = 1, 2, 3
SMALL_METHODS = ((OSD0, 0), (OSD_CS, 5), (OSD_CS, 48), (OSD_CS, 49), (OSD_CS, 64), (OSD_CS, 70), (OSD_E, 6))
TALL_METHODS = ((OSD0, 0), (OSD_CS, 3), (OSD_E, 3))

# k, words, kernel0 / kernelw: what the case is listed for (default dispatch, OSD-0 / higher order) -- checked against the matrix by
# tests/test_osd_bounds_cases.py; mq: osd_block_eliminate<MQ> of the tall ones; draw: syndromes drawn, of which the case keeps `rows`: those of `pick`, then in order
Case = namedtuple("Case", "id group m n dup seed p rows k words kernel0 kernelw what max_iter heavy mq pick prior draw row_extra")
Case.__new__.__defaults__ = (3, 0, None, (), (0.02, 0.12), 96, 3)


def _small(group, m, n, dup, k, kernel0, kernelw, what, seed=None, p=0.09, **kw):
    tag = f"{group}-{m}x{n}" + (f"-dup{dup}" if dup else "") + ("-heavy" if kw.get("heavy") else "")
    return Case(tag, group, m, n, dup, 100 * m + n + dup if seed is None else seed, p, 48 if m < 128 else 24 if m < 256 else 16, k, (n + 1 + 63) // 64, kernel0, kernelw, what, **kw)


def _rw(r, w, flat=None):
    return (f"osd0_flat_kernel<{flat[0]}, {flat[1]}>" if flat else f"osd0_reg_kernel<{r}, {w}>"), f"osdw_reg_kernel<{r}, {w}>"


RUNG_CASES = [
    _small("rung", 64, 127, 0, 63, *_rw(1, 2, (1, 5)), "rung <1, 2> full"),
    _small("rung", 65, 127, 0, 62, *_rw(2, 3, (2, 5)), "m one past <1, 2>"),
    _small("rung", 64, 128, 3, 67, *_rw(2, 3, (1, 5)), "n + 1 = 129: words 3, one past <1, 2>; rank-deficient", draw=3000, pick=(80, 546, 821)),
    _small("rung", 128, 191, 0, 63, *_rw(2, 3, (2, 8)), "rung <2, 3> full"),
    _small("rung", 128, 192, 0, 64, *_rw(2, 4, (2, 8)), "words 4: one past <2, 3>"),
    _small("rung", 128, 255, 2, 129, *_rw(2, 4, (2, 8)), "rung <2, 4> full; rank-deficient"),
    _small("rung", 129, 255, 0, 126, *_rw(4, 8), "m one past <2, 4>"),
    _small("rung", 128, 256, 0, 128, *_rw(4, 8, (2, 8)), "words 5: one past <2, 4>"),
    _small("rung", 256, 511, 0, 255, *_rw(4, 8), "rung <4, 8> full"),
    _small("rung", 257, 511, 0, 254, "osd0_kernel", "osdw_kernel", "m one past <4, 8>: the one-wavefront LDS kernels"),
    _small("rung", 256, 512, 1, 257, "osd0_kernel", "osdw_kernel", "words 9: one past <4, 8>; rank-deficient"),
    _small("rung", 3, 511, 0, 508, *_rw(4, 8), "three rows on the widest rung"),
    _small("rung", 100, 40, 0, 0, *_rw(2, 3, (2, 2)), "more checks than bits: 60 copied rows, k = 0"),
    _small("rung", 100, 40, 4, 4, *_rw(2, 3, (2, 2)), "more checks than bits, k = 4", draw=960, pick=(100, 232, 258)),
]
K_CASES = [
    _small("k", 64, 64, 0, 0, *_rw(1, 2, (1, 2)), "k = 0: the loop of its own; OSD_CS order clamped to 1", p=0.2),
    _small("k", 64, 65, 0, 1, *_rw(1, 2, (1, 3)), "k = 1", p=0.2, draw=960, pick=(22, 37, 58)),
    _small("k", 64, 96, 0, 32, *_rw(1, 2, (1, 3)), "k = 32: the upper half of the T record is cleared"),
    _small("k", 64, 97, 0, 33, *_rw(1, 2, (1, 5)), "k = 33: the upper half is written"),
    _small("k", 63, 127, 0, 64, *_rw(1, 2, (1, 5)), "k = 64: kwords still 1, k & 63 = 0"),
    _small("k", 62, 127, 0, 65, *_rw(1, 2, (1, 5)), "k = 65: kwords 2", seed=2, draw=3000, pick=(69, 1620)),
    _small("k", 62, 125, 2, 65, *_rw(1, 2, (1, 5)), "k = 65 on a rank-deficient matrix", draw=3000, pick=(1871,)),
    _small("k", 128, 255, 0, 127, *_rw(2, 4, (2, 8)), "k = 127", pick=(24, 30)),
    _small("k", 127, 256, 0, 129, *_rw(4, 8, (2, 8)), "k = 129: kwords 3"),
    _small("k", 129, 511, 0, 382, *_rw(4, 8), "k = 382: kwords 6"),
]
FLAT_CASES = [
    _small("flat", 65, 96, 0, 31, *_rw(2, 3, (2, 3)), "m one past R = 1, n = 96 exactly"),
    _small("flat", 128, 160, 0, 32, *_rw(2, 3, (2, 5)), "<2, 5> full"),
    _small("flat", 128, 161, 3, 36, *_rw(2, 3, (2, 8)), "n one past D = 5; rank-deficient"),
    _small("flat", 129, 256, 0, 127, *_rw(4, 8), "m one past the flat kernel", pick=(56, 59, 76)),
    _small("flat", 128, 257, 0, 129, *_rw(4, 8), "n one past the flat kernel"),
    _small("flat", 64, 96, 0, 32, *_rw(1, 2), "one row of 9 entries: back to osd0_reg_kernel", heavy=9, seed=6497),
]
# the shapes of the issue's groups that stand in another group already: 64x127, 128x255 (k), 128x256, 64x64, 64x97 (flat)
SMALL_CASES = RUNG_CASES + K_CASES + FLAT_CASES


def _tall(m, n, dup, mat_lds, what, kernel0=None, kernelw=None, **kw):
    hi = f"osd_big_kernel<true, {_b(mat_lds)}>"
    # (one BP iteration and very uneven priors: with the inputs of the small cases no candidate of order 3 beats the OSD-0 solution on matrices this tall)
    return Case(f"tall-{m}x{n}" + (f"-dup{dup}" if dup else ""), "tall", m, n, dup, 100 * m + n + dup, 0.09, 8 if m < 1536 else 4, n - m + dup, (n + 1 + 63) // 64,
                kernel0 or f"osd_big_kernel<false, {_b(mat_lds)}>", kernelw or hi, what, max_iter=1, prior=(0.005, 0.3), draw=16, mq=block_rows_per_thread(m), **kw)


TALL_CASES = [
    _tall(257, 400, 0, True, "MQ = 2, one row in the second register -- under set_osd_kernel(2): the default dispatch keeps so small a matrix on the one-wavefront kernels",
          kernel0="osd0_kernel", kernelw="osdw_kernel"),
    _tall(257, 1150, 0, True, "MQ = 2, one row in the second register, by default dispatch (18 words a row: beyond 40 KiB for one wavefront)"),
    _tall(512, 700, 0, True, "MQ = 2 full"),
    _tall(513, 700, 2, True, "MQ = 3, one row in the third register; rank-deficient"),
    _tall(768, 900, 0, True, "MQ = 3 full"),
    _tall(769, 900, 0, True, "MQ = 4, one row in the fourth register"),
    _tall(1024, 1200, 0, False, "MQ = 4 full"),
    _tall(1025, 1200, 0, False, "MQ = 6, one row in the fifth register"),
    _tall(1536, 1700, 0, False, "MQ = 6 full", pick=(5, 6)),
    _tall(1537, 1700, 0, False, "MQ = 8, one row in the seventh register", pick=(0, 4)),
    _tall(2048, 2200, 1, False, "MQ = 8 full; rank-deficient", pick=(4, 7, 10)),
    _tall(2049, 2200, 0, False, "beyond OSD_BLOCK_ROWS: the one-pivot-per-step loop by default dispatch", pick=(5, 13)),
]
ALL_CASES = SMALL_CASES + TALL_CASES
BY_ID = {c.id: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES)

# cases with k > 0 on which no input tried lets an OSD_CS / OSD_E candidate beat the OSD-0 solution: id -> what was tried (tests/test_osd_bounds_cases.py keeps
# the claim true: a listed case shows no win, every other one does)
WITHOUT_A_WIN = {
    "rung-3x511": "three checks: a candidate wins only where two or three set pivot bits add up to one lighter column, and BP's posteriors put that column "
                  "first already -- none in 960 syndromes on rows of 4 entries, none in 96 on rows of 43 or of 173",
}


def methods(case):
    return TALL_METHODS if case.group == "tall" else SMALL_METHODS


def reference_defined(case, method, order):
    """OSD_CS at an order beyond k writes past the reference's candidate strings (osd.hpp:90-99)."""
    return not (method == OSD_CS and order > case.k)


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """(h, copies, probs, syndromes) of a case: built once, shared (read-only)."""
    c = BY_ID[case_id]
    h, copies = bounds_code(c.m, c.n, c.seed, row_extra=c.row_extra, dup=c.dup, heavy=c.heavy)
    rng = np.random.default_rng(c.seed + 1)
    probs = rng.uniform(*c.prior, size=c.n)
    e = (rng.random((c.draw, c.n)) < c.p).astype(np.uint8)
    synd = np.asarray((h @ e.T % 2).T, dtype=np.uint8)
    if copies:  # a copy that disagrees with its original: outside the image
        synd[::5, copies[0][0]] ^= 1
    keep = list(c.pick) + [i for i in range(c.draw) if i not in c.pick]
    synd = np.ascontiguousarray(synd[keep[:c.rows]])
    for x in (probs, synd):
        x.setflags(write=False)
    return h, copies, probs, synd


def oracle_decode(case_id, method, order):
    """(decoding, iterations, converge) of the CPU checker."""
    import oracle
    c = BY_ID[case_id]
    h, _, probs, synd = inputs(case_id)
    with np.errstate(all="ignore"):
        o = oracle.BpOracle(h, error_channel=probs, max_iter=c.max_iter, bp_method="minimum_sum", ms_scaling_factor=ALPHA)
        dec, _, it, conv = o.bposd_decode_batch(synd, method, order, want_llr=False)
    return dec, it, conv


@functools.lru_cache(maxsize=None)
def expected(case_id, method, order):
    """What a decode of the case must return, computed once: the checker's (decoding, iterations, converge)."""
    out = oracle_decode(case_id, method, order)
    for x in out:
        x.setflags(write=False)
    return out
