"""Every selectable instantiation of the lane = edge kernels (bp_edge_kernel<R, UNIFORM, NOCLAMP>: 48; bp_edge8_kernel<R, DC, UNIFORM>: 36) and
every rung of the wavefront-per-syndrome ladders (bp_wave_kernel, bp_wave_ps_kernel; exact math), each on a smallest code that selects it
(tests/ladder_util.py; tests/test_ladder_cases.py checks the cases themselves without a GPU): the decode equals the oracle's bit for bit --
decisions, iteration counts, converge flags, log-ratios as bit patterns; the lane = edge cases also equal the lane = node kernel, mode 3 -- and
the launch log shows that EXACTLY the named instantiation ran and no other BP decode kernel did.  Just outside the bounds the log shows the
family was not used, and the bits still equal the oracle's."""
import numpy as np
import pytest

import ladder_util as lu
import launch_util

pytestmark = pytest.mark.gpu

_METHOD = {"product_sum": 0, "minimum_sum": 1}


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _decode(case, mode, switches):
    from ldpc_amd.engine import HipBpEngine
    h, probs, synd = lu.inputs(case.id)
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], probs, lu.MAX_ITER, _METHOD[case.method], case.alpha)
    try:
        eng.set_small_code_kernel(mode)
        for name, value in switches.items():
            eng.set_debug_switch(name, value)
        with launch_util.launch_log() as log:
            out = eng.decode_batch(synd)
    finally:
        eng.close()
    return out, log


def _same(got, want, who, method):
    for k, name in ((0, "decoding"), (2, "iterations"), (3, "converge")):
        assert np.array_equal(got[k], np.asarray(want[k]).astype(got[k].dtype)), f"{name}: {who}"
    differ = _bits(got[1]) != _bits(want[1])
    if method == "product_sum":  # (any NaN matches any NaN: the payload of inf - inf depends on the operand order -- oracle.bits_equal)
        differ &= ~(np.isnan(got[1]) & np.isnan(want[1]))
    assert not differ.any(), f"log-ratios (bit patterns): {who}: {int(differ.sum())} of {differ.size} differ, first at {tuple(np.argwhere(differ)[0])}"


def _check(case, node_kernel_too):
    got, log = _decode(case, case.mode, case.switches)
    _same(got, lu.expected(case.id), "kernel vs oracle", case.method)
    if node_kernel_too:
        node, node_log = _decode(case, 3, {})
        _same(got, node, "kernel vs node kernel (mode 3)", case.method)
        launch_util.assert_ran(node_log, "bp_wave_kernel")
    launch_util.assert_resolved(log)
    ran = launch_util.of(log, *lu.BP_DECODE_KERNELS)
    if case.id in lu.UNREACHABLE:
        assert case.kernel not in ran, f"{case.kernel} ran, but is listed as unreachable: {lu.UNREACHABLE[case.id]}"
    elif case.kernel:
        assert ran == [case.kernel], f"expected exactly {case.kernel}"
        assert log[case.kernel] == 1
    assert ran, "no BP decode kernel in the log"
    launch_util.assert_not_ran(log, *(case.absent or ()))


@pytest.mark.parametrize("case", lu.EDGE_CASES, ids=[c.id for c in lu.EDGE_CASES])
def test_edge_kernel_instantiation(case, oracle_built):
    _check(case, True)


@pytest.mark.parametrize("case", lu.EDGE8_CASES, ids=[c.id for c in lu.EDGE8_CASES])
def test_edge8_kernel_instantiation(case, oracle_built):
    _check(case, True)


@pytest.mark.parametrize("case", lu.OUTSIDE_CASES, ids=[c.id for c in lu.OUTSIDE_CASES])
def test_just_outside_the_bounds(case, oracle_built):
    _check(case, True)


@pytest.mark.parametrize("case", lu.WAVE_CASES, ids=[c.id for c in lu.WAVE_CASES])
def test_wave_kernel_rung(case, oracle_built):
    _check(case, False)


@pytest.mark.parametrize("case", lu.WAVE_PS_CASES, ids=[c.id for c in lu.WAVE_PS_CASES])
def test_wave_ps_kernel_rung(case, oracle_built):
    _check(case, False)
