"""Shared by tests/test_ladder_cases.py (CPU) and tests/test_gpu_instantiations.py (GPU): seeded random parity-check matrices with EXACTLY
the stated shape -- m rows, a heaviest row, a heaviest column, a lightest row, every column present -- and the case tables that name, for
every selectable instantiation of the lane = edge kernels (bp_edge_kernel, bp_edge8_kernel) and of the wavefront-per-syndrome kernels
(bp_wave_kernel, bp_wave_ps_kernel), a smallest code that selects it.  The expected kernel names are written out here from the size rules
of ldpc_amd/csrc/host_onchip.h (plan_edge, plan_edge8, pick_wave, pick_wave_ps); nothing is imported from the library.

Inputs of every case: 131 syndromes (no multiple of 64 or of a pull chunk) of errors at p = 0.08 unless the case says otherwise, max_iter 8,
row 0 all zero, one syndrome byte 2 (row 5) and one 3 (row 6: parity from bit 0, neither row converges -- bp.hpp:236, :300); per-column-prior
cases draw their priors in 0.01 .. 0.15 and get one p = 0.5 (prior 0.0) and one p = 0.7 (negative prior); the wavefront cases on (4,4) and (8,8)
codes take p = 0.12 and the others p = 0.04, where the oracle converges on some rows and not on others (tests/test_ladder_cases.py)."""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

BATCH = 131
MAX_ITER = 8
BAD_ROWS = (5, 6)


def build_member(seed, m, max_row, max_col, min_row=1, base_row=None, base_col=None, n=None, empty_cols=0):
    """A seeded random m x n matrix: one row of exactly max_row entries, one of exactly min_row, the others min_row .. base_row (default
    max_row); one column of exactly max_col entries, the others 1 .. base_col (default max_col); `empty_cols` columns without entries are
    appended.  n: aimed at when given, else drawn; always inside what the sockets allow.  Rows never repeat a column."""
    base_row = max_row if base_row is None else base_row
    base_col = max_col if base_col is None else base_col
    assert 1 <= min_row <= base_row <= max_row and 1 <= base_col <= max_col and m >= max_col and (m >= 2 or min_row == max_row)
    rng = np.random.default_rng(seed)
    for _ in range(2000):
        w = rng.integers(min_row, base_row + 1, size=m)
        heavy, light = (int(x) for x in rng.choice(m, size=2, replace=False)) if m >= 2 else (0, 0)
        w[light] = min_row
        w[heavy] = max_row
        s = int(w.sum())
        # columns: 1 .. base_col entries each, column `big` exactly max_col, summing to s
        lo, hi = -(-(s - max_col) // base_col) + 1, s - max_col + 1
        if lo > hi:
            continue
        if n is None:
            want = int(round(s / rng.uniform(1.25, 0.5 + 0.5 * max(base_col, 2.0))))
        else:
            want = n
        cols = min(max(want, lo, max_row), hi)
        if cols < max_row:
            continue
        deg = np.ones(cols, np.int64)
        big = int(rng.integers(cols))
        deg[big] = max_col
        for _ in range(s - int(deg.sum())):
            room = np.flatnonzero((deg < base_col) & (np.arange(cols) != big))
            deg[int(rng.choice(room))] += 1
        sockets = np.repeat(np.arange(cols), deg)
        rng.shuffle(sockets)
        # rows take their sockets in order; a socket that would repeat a column in its row is swapped with a later one that does not
        ok, at = True, 0
        for i in range(m):
            for k in range(at, at + int(w[i])):
                if sockets[k] in sockets[at:k]:
                    later = [q for q in range(at + int(w[i]), s) if sockets[q] not in sockets[at:k]]
                    if not later:
                        ok = False
                        break
                    q = int(rng.choice(later))
                    sockets[k], sockets[q] = sockets[q], sockets[k]
            if not ok:
                break
            at += int(w[i])
        if not ok:
            continue
        h = np.zeros((m, cols + empty_cols), np.uint8)
        at = 0
        for i in range(m):
            h[i, sockets[at:at + int(w[i])]] = 1
            at += int(w[i])
        if (h.sum(axis=1) == w).all() and (h[:, :cols].sum(axis=0) == deg).all():
            return sp.csr_matrix(h)
    raise AssertionError(f"no member found: seed {seed}, m {m}, rows {min_row}..{max_row}, columns ..{max_col}")


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
# kernel: the one BP decode kernel the launch log must show (None: see `absent`); absent: kernel base names the log must NOT show
Case = namedtuple("Case", "id kernel absent method alpha mode switches uniform p seed build prior_draw zero_prior")
Case.__new__.__defaults__ = (None,) * len(Case._fields)

# every kernel base name that decodes BP on the parallel schedule: a case's log shows exactly ONE instantiation among them
BP_DECODE_KERNELS = ("bp_edge_kernel", "bp_edge8_kernel", "bp_wave_kernel", "bp_wave_ps_kernel", "bp_small_kernel", "bp_decode_kernel",
                     "bp_spread_check_kernel", "bp_spread_bit_kernel", "bp_spread_init_kernel", "bp_spread_finish_kernel", "bp_spread_synd_kernel",
                     "bp_f32_check_kernel", "bp_f32_bit_kernel")


def edge_rounds(m):
    """plan_edge: four lanes a row, 64 lanes a round."""
    return (4 * m + 63) // 64


EDGE8_ROUNDS = {3: (2, 3, 4, 5, 6, 7, 8, 9, 10, 12), 4: (2, 3, 4, 5, 6, 7, 8, 9)}


def edge8_rounds(m, dc):
    """plan_edge8: eight lanes a row; the smallest compiled R that holds them (0: none does)."""
    need = (8 * m + 63) // 64
    return next((r for r in EDGE8_ROUNDS[dc] if r >= need), 0)


def _b(x):
    return "true" if x else "false"


def _edge_cases():
    out = []
    for r in range(1, 17):
        for m in (16 * (r - 1) + 1, 16 * r):
            for form in ("percol", "noclamp", "clamp"):
                # (m = 1: no column can have two entries -- one weight-4 row; the clamped form wants a weight-1 row, so two rows at least: m = 1 gets it from EDGE_CLAMP)
                one = m == 1
                kw = dict(m=m, max_row=4, max_col=1 if one else 2, min_row=4 if one else 2 if form == "noclamp" else 1)
                name = f"bp_edge_kernel<{r}, {_b(form != 'percol')}, {_b(form == 'noclamp')}>"
                # (a ONE-row code converges on every syndrome when one prior is 0.0, or when the weakest prior is below 0.625 of the others: the flipped
                #  bit always satisfies the only check.  So m = 1 with per-column priors keeps the p = 0.7 but not the p = 0.5, and draws the rest
                #  in 0.3 .. 0.4 -- then its zero syndromes do not converge, its others do)
                out.append(Case(id=f"edge-R{r}-m{m}-{form}", kernel=name, method="minimum_sum", alpha=0.625, mode=6,
                                switches={"EDGE_CLAMP": 1} if one and form == "clamp" else {}, uniform=form != "percol", p=0.08,
                                seed=1000 + 10 * m + ("percol", "noclamp", "clamp").index(form), build=kw,
                                prior_draw=(0.3, 0.4) if one else None, zero_prior=not one))
    kw = dict(m=256, max_row=4, max_col=2, min_row=2)
    out.append(Case(id="edge-R16-adaptive-alpha", kernel="bp_edge_kernel<16, true, true>", method="minimum_sum", alpha=0.0, mode=6, switches={},
                    uniform=True, p=0.08, seed=4001, build=kw))
    out.append(Case(id="edge-R16-alpha-above-1", kernel="bp_edge_kernel<16, true, false>", method="minimum_sum", alpha=1.25, mode=6, switches={},
                    uniform=True, p=0.08, seed=4002, build=kw))
    return out


def _edge8_cases():
    out = []
    for dc in (3, 4):
        prev = 0
        for r in EDGE8_ROUNDS[dc]:
            # both ends of the R's range: 8 R_prev + 1 rows (the first R: as few rows as a column of dc entries needs) and 8 R
            for m in (max(8 * prev + 1, dc), 8 * r):
                for uniform in (True, False):
                    out.append(Case(id=f"edge8-DC{dc}-R{r}-m{m}-{'uniform' if uniform else 'percol'}", kernel=f"bp_edge8_kernel<{r}, {dc}, {_b(uniform)}>",
                                    method="minimum_sum", alpha=0.625, mode=6, switches={}, uniform=uniform, p=0.08,
                                    seed=5000 + 100 * dc + 2 * m + int(uniform), build=dict(m=m, max_row=8, max_col=dc, min_row=1)))
            prev = r
    return out


def _outside_cases():
    edge_family = ("bp_edge_kernel", "bp_edge8_kernel")
    mk = lambda id, kernel, absent, seed, **kw: Case(id=id, kernel=kernel, absent=absent, method="minimum_sum", alpha=0.625, mode=6, switches={},
                                                     uniform=True, p=0.08, seed=seed, build=kw)
    return [
        mk("outside-m257", None, edge_family, 6001, m=257, max_row=4, max_col=2),
        mk("outside-weight5-row", "bp_edge8_kernel<5, 3, true>", ("bp_edge_kernel",), 6002, m=40, max_row=5, base_row=4, max_col=2),
        mk("outside-weight3-column", "bp_edge8_kernel<5, 3, true>", ("bp_edge_kernel",), 6003, m=40, max_row=4, max_col=3, base_col=2),
        mk("outside-m97-dc3", None, edge_family, 6004, m=97, max_row=8, max_col=3),
        mk("outside-m73-dc4", None, edge_family, 6005, m=73, max_row=8, max_col=4),
        mk("outside-weight9-row", None, edge_family, 6006, m=40, max_row=9, base_row=8, max_col=3),
        mk("outside-weight5-column", None, edge_family, 6007, m=40, max_row=8, max_col=5, base_col=4),
        mk("outside-empty-column", None, edge_family, 6008, m=40, max_row=4, max_col=2, empty_cols=1),
    ]


_METHOD_ID = {"product_sum": 0, "minimum_sum": 1}  # ldpc::bp::BpMethod (bp.hpp:23-26): the kernels' METHOD argument


def _wave_cases():
    """Each rung of pick_wave AT its bound: modes 4 (a wavefront per syndrome) and 5 (a team per syndrome), exact math.
    What the names can tell apart at 131 syndromes: mode 4 from the default plan everywhere (so small a batch takes the team form by
    itself); mode 5 from the default DISPATCH where that prefers another family -- min-sum (4,2) and (6,3): the lane = edge kernels, product-sum
    up to (8,4): bp_wave_ps_kernel -- but not on the other five rungs, where the default dispatch and plan give the team form too."""
    out = []
    for method in ("minimum_sum", "product_sum"):
        for dr, dc in ((4, 2), (4, 4), (6, 3), (8, 4), (8, 8), (16, 8)):
            if (dr, dc) == (16, 8) and method == "product_sum":
                continue  # (pick_wave: min-sum only)
            for mode in (4, 5):
                out.append(Case(id=f"wave-{method}-{dr}x{dc}-mode{mode}", kernel=f"bp_wave_kernel<{_METHOD_ID[method]}, 0, {dr}, {dc}, {_b(mode == 5)}>",
                                method=method, alpha=0.625 if method == "minimum_sum" else 1.0, mode=mode, switches={}, uniform=(dr + mode) % 2 == 0,
                                p=0.12 if dr == dc else 0.04, seed=7000 + 10 * dr + dc, build=dict(m=round(150 * (1 + dc) / (1 + dr)), max_row=dr, max_col=dc, min_row=1, n=150)))
    return out


def _wave_ps_cases():
    """Each rung of pick_wave_ps at its bound: mode 1 with PS_TEAM 0 / 1, exact math."""
    out = []
    for dr, dc in ((4, 2), (4, 4), (6, 3), (8, 4), (16, 8), (32, 8)):
        for team in (0, 1):
            out.append(Case(id=f"wave_ps-{dr}x{dc}-team{team}", kernel=f"bp_wave_ps_kernel<0, {dr}, {dc}, {_b(team)}>", method="product_sum", alpha=1.0,
                            mode=1, switches={"PS_TEAM": team}, uniform=(dr + team) % 2 == 0, p=0.12 if dr == dc else 0.04, seed=8000 + 10 * dr + dc,
                            build=dict(m=round(150 * (1 + dc) / (1 + dr)), max_row=dr, max_col=dc, min_row=1, n=150)))
    return out


EDGE_CASES = _edge_cases()
EDGE8_CASES = _edge8_cases()
OUTSIDE_CASES = _outside_cases()
WAVE_CASES = _wave_cases()
WAVE_PS_CASES = _wave_ps_cases()
ALL_CASES = EDGE_CASES + EDGE8_CASES + OUTSIDE_CASES + WAVE_CASES + WAVE_PS_CASES

# (rung, team) combinations of the wavefront kernels that no mode reaches because the plan declines them: id of the case above -> the
# reason.  The GPU test asserts from the log that such a case does NOT launch the named instantiation, so the claim stays true.
UNREACHABLE = {}


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """(h, probs, syndromes) of a case: built once, shared by every test that needs them (treat as read-only)."""
    c = next(c for c in ALL_CASES if c.id == case_id)
    h = build_member(c.seed, **c.build)
    m, n = h.shape
    rng = np.random.default_rng(c.seed + 1)
    if c.uniform:
        probs = np.full(n, c.p)
    else:
        probs = rng.uniform(*(c.prior_draw or (0.01, 0.15)), size=n)
        a, b = (int(x) for x in rng.choice(n, size=2, replace=False))
        probs[b] = 0.7
        if c.zero_prior is not False:
            probs[a] = 0.5
    e = (rng.random((BATCH, n)) < c.p).astype(np.uint8)
    synd = np.ascontiguousarray((h @ e.T % 2).T.astype(np.uint8))
    synd[0] = 0
    synd[BAD_ROWS[0], int(rng.integers(m))] = 2
    synd[BAD_ROWS[1], int(rng.integers(m))] = 3
    for x in (probs, synd):
        x.setflags(write=False)
    return h, probs, synd


@functools.lru_cache(maxsize=None)
def expected(case_id):
    """The oracle's (decoding, llr, iterations, converge) of a case: computed once."""
    import oracle
    c = next(c for c in ALL_CASES if c.id == case_id)
    h, probs, synd = inputs(case_id)
    with np.errstate(all="ignore"):
        return oracle.BpOracle(h, error_channel=probs, max_iter=MAX_ITER, bp_method=c.method, ms_scaling_factor=c.alpha).decode_batch(synd)
