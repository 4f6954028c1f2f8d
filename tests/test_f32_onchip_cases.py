"""What tests/test_gpu_f32_onchip.py relies on, checked without a GPU: the float32 kernel name of every ladder case (the FP64 name of
tests/ladder_util.py renamed -- the two dtypes share plan_edge and plan_edge8), and that the float32 restatement of every case has rows
that converge, rows that do not, and no NaN among its posteriors (the GPU test poisons its outputs with NaN)."""
import re

import numpy as np
import pytest

import f32_onchip_util as ou
import ladder_util as lu


def test_kernel_names_are_the_fp64_names_renamed():
    names = [ou.f32_kernel_name(c.kernel) for c in ou.CASES]
    for c, name in zip(ou.CASES, names):
        if c.kernel is None:
            assert name is None
            continue
        assert re.fullmatch(r"bp_edge_f32_kernel<\d+, (true|false), (true|false)>|bp_edge8_f32_kernel<\d+, [34], (true|false)>", name), name
        assert name.split("<")[1] == c.kernel.split("<")[1] and name != c.kernel
    assert ou.f32_kernel_name("bp_edge_kernel<16, true, true>") == "bp_edge_f32_kernel<16, true, true>"
    assert ou.f32_kernel_name("bp_edge8_kernel<9, 3, true>") == "bp_edge8_f32_kernel<9, 3, true>"
    # every instantiation of the two ladders is named by some case: 48 + 36
    onchip = {ou.f32_kernel_name(c.kernel) for c in ou.ONCHIP_CASES}
    assert len([k for k in onchip if k.startswith("bp_edge_f32_kernel<")]) == 48
    assert len([k for k in onchip if k.startswith("bp_edge8_f32_kernel<")]) == 36
    # the two cases that fall from bp_edge to bp_edge8
    fall = [ou.f32_kernel_name(c.kernel) for c in lu.OUTSIDE_CASES if c.kernel]
    assert fall == ["bp_edge8_f32_kernel<5, 3, true>"] * 2


@pytest.mark.parametrize("case", ou.CASES, ids=[c.id for c in ou.CASES])
def test_case_has_converging_and_unconverging_rows_and_no_nan(case):
    dec, llr, it, cv = ou.expected(case.id)
    assert cv.any(), "no row converges"
    assert (~cv).any(), "every row converges"
    assert not np.isnan(llr).any(), "a NaN posterior"
    assert np.array_equal(llr, llr.astype(np.float32).astype(np.float64))
    assert it.min() >= 1 and it.max() <= lu.MAX_ITER
