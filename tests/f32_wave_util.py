"""Shared by tests/test_f32_wave_cases.py (CPU) and tests/test_gpu_f32_wave.py (GPU): the lane = node kernel of the float32 message mode
(ldpc_amd/csrc/bp_wave_f32_kernel.h, switched on with ldpc_hip_bp_set_f32_lane_node) on a smallest code for each of its twelve
instantiations, and the float32 restatement (tests/f32_util.py) of every case, computed once per process and shared (treat as read-only).

The cases: the twelve min-sum entries of ladder_util.WAVE_CASES -- the six rungs (rows <=, columns <=) of the lane = node ladder AT their
bounds, under small-code kernel modes 4 (a wavefront per syndrome) and 5 (a team per syndrome), n = 150, 131 syndromes, max_iter 8, an
all-zero row, a syndrome byte 2 and a byte 3 -- and two added ones:
  * a (4,2)-rung code with n = 300 under mode 4: 320 padded columns are TWO rounds of a wavefront's bit pass at U = 4 columns per lane;
  * a (16,8)-rung code under mode -1: the plan's own choice, which for 131 syndromes is the team form (no more syndromes than wavefront slots).
The kernel names are written out here from the rules of ldpc_amd/csrc/host_onchip.h (LDPC_WAVE_LADDER: a code takes the first rung that holds
it; mode 4 / 5: TEAM false / true); nothing is imported from the library."""
import functools
from collections import namedtuple

import numpy as np

import f32_util as fu
import ladder_util as lu

# what the float32 per-pass route launches every iteration / the template of the lane = node float32 kernel / the lane = edge float32 templates
PER_PASS = ("bp_f32_check_kernel", "bp_f32_bit_kernel")
ONCHIP_WAVE = ("bp_wave_f32_kernel",)
ONCHIP_EDGE = ("bp_edge_f32_kernel", "bp_edge8_f32_kernel")

RUNGS = ((4, 2), (4, 4), (6, 3), (8, 4), (8, 8), (16, 8))  # LDPC_WAVE_LADDER, ascending

# id; the rung; the small-code kernel mode; TEAM; alpha; ladder: the ladder_util case whose inputs it takes, or None: `build`, `p`, `seed`, `uniform`
WCase = namedtuple("WCase", "id dr dc mode team alpha ladder build p seed uniform")
WCase.__new__.__defaults__ = (None,) * len(WCase._fields)


def rung_of(max_row, max_col):
    """The first rung that holds rows of max_row and columns of max_col entries (None: none does)."""
    return next(((r, c) for r, c in RUNGS if max_row <= r and max_col <= c), None)


def kernel_name(dr, dc, team):
    return f"bp_wave_f32_kernel<{dr}, {dc}, {'true' if team else 'false'}>"


def route_name(team):
    """What ldpc_hip_bp_f32_route / HipBpEngine.f32_route answer for the lane = node kernel."""
    return "bp_wave_team" if team else "bp_wave"


def _cases():
    out = []
    for c in lu.WAVE_CASES:
        if c.method != "minimum_sum":
            continue
        dr, dc = c.build["max_row"], c.build["max_col"]
        assert rung_of(dr, dc) == (dr, dc) and c.mode in (4, 5)
        out.append(WCase(id=c.id.replace("wave-minimum_sum", "wave_f32"), dr=dr, dc=dc, mode=c.mode, team=c.mode == 5, alpha=c.alpha, ladder=c.id))
    assert len(out) == 12
    out.append(WCase(id="wave_f32-4x2-n300-two-rounds-mode4", dr=4, dc=2, mode=4, team=False, alpha=0.625,
                     build=dict(m=180, max_row=4, max_col=2, min_row=1, n=300), p=0.04, seed=9142, uniform=False))
    out.append(WCase(id="wave_f32-16x8-default-mode", dr=16, dc=8, mode=-1, team=True, alpha=0.625,
                     build=dict(m=79, max_row=16, max_col=8, min_row=1, n=150), p=0.04, seed=9168, uniform=True))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
DEFAULT_MODE_CASE = "wave_f32-16x8-default-mode"


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """(h, probs, syndromes) of a case, built once (read-only).  The added cases follow ladder_util.inputs: 131 syndromes of errors at p,
    row 0 all zero, a byte 2 in row 5 and a byte 3 in row 6; per-column priors in 0.01 .. 0.15 with one p = 0.5 and one p = 0.7."""
    c = BY_ID[case_id]
    if c.ladder:
        return lu.inputs(c.ladder)
    h = lu.build_member(c.seed, **c.build)
    m, n = h.shape
    rng = np.random.default_rng(c.seed + 1)
    if c.uniform:
        probs = np.full(n, c.p)
    else:
        probs = rng.uniform(0.01, 0.15, size=n)
        a, b = (int(x) for x in rng.choice(n, size=2, replace=False))
        probs[a], probs[b] = 0.5, 0.7
    e = (rng.random((lu.BATCH, n)) < c.p).astype(np.uint8)
    synd = np.ascontiguousarray((h @ e.T % 2).T.astype(np.uint8))
    synd[0] = 0
    synd[lu.BAD_ROWS[0], int(rng.integers(m))] = 2
    synd[lu.BAD_ROWS[1], int(rng.integers(m))] = 3
    for x in (probs, synd):
        x.setflags(write=False)
    return h, probs, synd


@functools.lru_cache(maxsize=None)
def expected(case_id, dtype=np.float32):
    """The restatement's (decoding, llr widened, iterations, converge) of a case at the given message dtype."""
    h, probs, synd = inputs(case_id)
    out = fu.min_sum_restatement(h, probs, synd, lu.MAX_ITER, BY_ID[case_id].alpha, dtype)
    for x in out:
        x.setflags(write=False)
    return out


def case_dict(case_id, max_iter=lu.MAX_ITER):
    """A case in the shape of f32_util's cases."""
    h, probs, synd = inputs(case_id)
    return dict(h=h, probs=probs, synd=synd, max_iter=max_iter, alpha=BY_ID[case_id].alpha)
