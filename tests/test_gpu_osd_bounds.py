"""The OSD kernels AT the bounds of the shapes that select their code (tests/osd_bounds_util.py has the cases and says what each is for): the rungs of
osd0_reg_kernel<R, W> / osdw_reg_kernel<R, W> full and one step past, k = n - rank H around the half-word and word steps of osdw_reg_kernel's T records,
the bounds of osd0_flat_kernel<R, D>, and the heights at which osd_big_kernel changes its osd_block_eliminate<MQ> -- a device function the launch log
cannot name, so a matrix of that height is the only witness -- up to 2049 rows, where the one-pivot-per-step loop takes over with no switch set.

Per decode: decisions, converge flags and iteration counts bit for bit against the CPU checker, the status bytes against H x = s, and the launched
OSD kernel -- read from the launch log, the second pass over the rows outside the image included -- against the restated choice of plan_osd."""
import numpy as np
import pytest

import launch_util
import osd_bounds_util as u

pytestmark = pytest.mark.gpu

OSD_KERNELS = ("osd0_flat_kernel", "osd0_reg_kernel", "osdw_reg_kernel", "osd0_kernel", "osdw_kernel", "osd_big_kernel")


def _engine(case_id):
    from ldpc_amd.engine import HipBpEngine
    c = u.BY_ID[case_id]
    h, copies, probs, synd = u.inputs(case_id)
    return HipBpEngine(h.indptr, h.indices, c.n, probs, c.max_iter, 1, u.ALPHA), h, copies, synd


def _decode_and_check(eng, h, copies, synd, want, kernel, what):
    """One BP + OSD decode with the engine's present settings: outputs, status bytes and the launched OSD kernel."""
    dec, it, conv = want
    with launch_util.launch_log() as log:
        got = eng.decode_batch(synd, want_llr=False, osd=True)
    launch_util.assert_resolved(log)
    assert np.array_equal(got[3], conv) and np.array_equal(got[2], it), what
    bad = np.flatnonzero((got[0] != dec).any(axis=1))
    assert not len(bad), f"{what}: rows {bad.tolist()} differ from the checker"
    solves = np.all((got[0].astype(np.int64) @ h.T.toarray().astype(np.int64)) % 2 == synd, axis=1)
    assert np.array_equal(eng.osd_status(len(synd)), np.where(conv, 0, np.where(solves, 1, 2))), what
    # a rank-deficient H: osd_exact_kernel and a second pass through the SAME kernel (both sized on the device: launched whether rows need them or not)
    passes = 2 if copies else 1
    assert {k: log[k] for k in launch_util.of(log, *OSD_KERNELS)} == {kernel: passes}, f"{what}: {sorted(log)}"
    assert bool(launch_util.of(log, "osd_exact_kernel")) == bool(copies), what
    return solves


SMALL = [(c.id, meth, order) for c in u.SMALL_CASES for meth, order in u.methods(c)]


@pytest.mark.parametrize("case_id,method,order", SMALL, ids=[f"{c}-{('', 'osd0', 'e', 'cs')[m]}{o}" for c, m, o in SMALL])
def test_small_shapes_at_their_bounds(case_id, method, order, oracle_built):
    c = u.BY_ID[case_id]
    want = u.expected(case_id, method, order)
    eng, h, copies, synd = _engine(case_id)
    deg = int(np.diff(h.indptr).max())
    higher = method != u.OSD0
    eng.set_osd(method, order)
    # (the table's names are the default dispatch's: the case is run where it was listed for)
    assert u.expected_kernel(c.m, c.n, deg, higher, -1) == (c.kernelw if higher else c.kernel0)
    outside = 0
    for mode in (-1, 0, 2):
        eng.set_osd_kernel(mode)
        kernel = u.expected_kernel(c.m, c.n, deg, higher, mode)
        solves = _decode_and_check(eng, h, copies, synd, want, kernel, f"{case_id} {method}/{order} osd kernel {mode}")
        outside = int((~solves).sum())
        if kernel.startswith("osd0_flat_kernel"):
            eng.set_debug_switch("OSD_NO_FLAT", 1)
            _decode_and_check(eng, h, copies, synd, want, u.expected_kernel(c.m, c.n, deg, higher, mode, no_flat=True), f"{case_id} OSD_NO_FLAT")
            eng.set_debug_switch("OSD_NO_FLAT", -1)
    assert (outside > 0) == bool(copies), "rank-deficient cases carry syndromes outside the image, the others none"
    eng.close()


TALL = [(c.id, meth, order) for c in u.TALL_CASES for meth, order in u.methods(c)]
PLANES_CASE = "tall-769x900"  # OSD_PLANES 1: one wavefront weighs the candidates


@pytest.mark.parametrize("case_id,method,order", TALL, ids=[f"{c}-{('', 'osd0', 'e', 'cs')[m]}{o}" for c, m, o in TALL])
def test_tall_shapes_through_the_workgroup_kernel(case_id, method, order, oracle_built):
    c = u.BY_ID[case_id]
    want = u.expected(case_id, method, order)
    eng, h, copies, synd = _engine(case_id)
    deg = int(np.diff(h.indptr).max())
    higher = method != u.OSD0
    eng.set_osd(method, order)
    kernel = u.expected_kernel(c.m, c.n, deg, higher, -1)  # no switch set: 2049 rows reach the one-pivot-per-step loop by themselves
    assert kernel == (c.kernelw if higher else c.kernel0)
    _decode_and_check(eng, h, copies, synd, want, kernel, f"{case_id} {method}/{order}")
    if not kernel.startswith("osd_big_kernel"):  # (257 x 400 is small enough for the one-wavefront kernels: its 257th row reaches osd_block_eliminate<2> so)
        eng.set_osd_kernel(2)
        kernel = u.expected_kernel(c.m, c.n, deg, higher, 2)
        _decode_and_check(eng, h, copies, synd, want, kernel, f"{case_id} {method}/{order} osd kernel 2")
    assert kernel.startswith("osd_big_kernel<")
    if case_id == PLANES_CASE and higher:
        eng.set_debug_switch("OSD_PLANES", 1)
        _decode_and_check(eng, h, copies, synd, want, kernel, f"{case_id} {method}/{order} OSD_PLANES 1")
    eng.close()
