"""Shared by tests/test_f32_onchip_cases.py (CPU) and tests/test_gpu_f32_onchip.py (GPU): the float32 on-chip kernels
(ldpc_amd/csrc/bp_edge_f32_kernel.h) on the cases of tests/ladder_util.py -- the expected float32 kernel name of every case, and the
float32 restatement (tests/f32_util.py) of every case, computed once per process and shared (treat as read-only)."""
import functools

import numpy as np

import f32_util as fu
import ladder_util as lu

# what the float32 per-pass route launches every iteration, and the two on-chip float32 templates
PER_PASS = ("bp_f32_check_kernel", "bp_f32_bit_kernel")
ONCHIP = ("bp_edge_f32_kernel", "bp_edge8_f32_kernel")


def f32_kernel_name(kernel):
    """The float32 instantiation a case must launch: its FP64 kernel renamed; None stays None (the per-pass route)."""
    if kernel is None:
        return None
    for old, new in (("bp_edge8_kernel<", "bp_edge8_f32_kernel<"), ("bp_edge_kernel<", "bp_edge_f32_kernel<")):
        if kernel.startswith(old):
            return new + kernel[len(old):]
    raise AssertionError(f"not a lane = edge kernel: {kernel}")


ONCHIP_CASES = lu.EDGE_CASES + lu.EDGE8_CASES
CASES = ONCHIP_CASES + lu.OUTSIDE_CASES
_BY_ID = {c.id: c for c in CASES}


@functools.lru_cache(maxsize=None)
def expected(case_id):
    """The float32 restatement's (decoding, llr widened, iterations, converge) of a ladder case."""
    c = _BY_ID[case_id]
    h, probs, synd = lu.inputs(case_id)
    out = fu.min_sum_restatement(h, probs, synd, lu.MAX_ITER, c.alpha, np.float32)
    for x in out:
        x.setflags(write=False)
    return out


def case_dict(case_id, max_iter=lu.MAX_ITER):
    """A ladder case in the shape of f32_util's cases."""
    h, probs, synd = lu.inputs(case_id)
    return dict(h=h, probs=probs, synd=synd, max_iter=max_iter, alpha=_BY_ID[case_id].alpha)
