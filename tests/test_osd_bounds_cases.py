"""The cases of tests/osd_bounds_util.py, checked without a GPU: every case has the rank, the k = n - rank, the words of [H | s] and the kernel it is
listed for; the CPU checker equals the real reference on every (method, order) the GPU test runs and the reference defines; and every case shows what it
is for -- rows that reach OSD, rows on which a higher-order candidate beats the OSD-0 solution, rows on which an OSD_CS pair reaching past the 64th
non-pivot column wins, rows outside the image where H is rank-deficient."""
import numpy as np
import pytest

import oracle
import osd_bounds_util as u

IDS = [c.id for c in u.ALL_CASES]


def test_the_table_holds_every_bound():
    shapes = {(c.group, c.m, c.n) for c in u.ALL_CASES}
    for m, n in ((64, 127), (65, 127), (64, 128), (128, 191), (128, 192), (128, 255), (129, 255), (128, 256), (256, 511), (257, 511), (256, 512), (3, 511), (100, 40)):
        assert ("rung", m, n) in shapes
    ks = {(c.m, c.n): c.k for c in u.ALL_CASES if c.dup == 0}
    for (m, n), k in {(64, 64): 0, (64, 65): 1, (64, 96): 32, (64, 97): 33, (64, 127): 63, (63, 127): 64, (62, 127): 65, (128, 255): 127, (128, 256): 128,
                      (127, 256): 129, (129, 511): 382}.items():
        assert ks[(m, n)] == k
    for m, n in ((64, 64), (65, 96), (64, 97), (128, 160), (128, 161), (128, 256), (129, 256), (128, 257)):
        assert any((c.m, c.n) == (m, n) for c in u.SMALL_CASES)
    assert any(c.heavy == 9 and (c.m, c.n) == (64, 96) for c in u.SMALL_CASES)
    for m, n in ((257, 400), (257, 1150), (512, 700), (513, 700), (768, 900), (769, 900), (1024, 1200), (1025, 1200), (1536, 1700), (1537, 1700), (2048, 2200), (2049, 2200)):
        assert ("tall", m, n) in shapes
    # every instantiation of the small-matrix kernels is some case's default dispatch (osd0_reg_kernel<2, 3> and <2, 4>: under OSD_NO_FLAT, which the GPU
    # test sets wherever the flat kernel applies -- rows of up to eight entries on these shapes always take that), every MQ of osd_block_eliminate some tall case's
    names = {c.kernel0 for c in u.ALL_CASES} | {c.kernelw for c in u.ALL_CASES} | {u.expected_kernel(c.m, c.n, 6, False, -1, no_flat=True) for c in u.SMALL_CASES}
    for r, w in ((1, 2), (2, 3), (2, 4), (4, 8)):
        assert {f"osd0_reg_kernel<{r}, {w}>", f"osdw_reg_kernel<{r}, {w}>"} <= names
    assert {f"osd0_flat_kernel<{r}, {d}>" for r in (1, 2) for d in (2, 3, 5, 8)} - names <= {"osd0_flat_kernel<1, 8>"}  # (tests/test_gpu_osd_flat.py has it)
    assert {"osd0_kernel", "osdw_kernel"} <= names and {f"osd_big_kernel<{a}, {b}>" for a in ("false", "true") for b in ("false", "true")} <= names
    assert {c.mq for c in u.TALL_CASES} == {2, 3, 4, 6, 8, 0}
    for group in ("rung", "k", "flat", "tall"):
        assert any(c.group == group and u.inputs(c.id)[1] for c in u.ALL_CASES), f"{group}: no rank-deficient case"


@pytest.mark.parametrize("case_id", IDS)
def test_case_is_what_it_is_listed_for(case_id):
    c = u.BY_ID[case_id]
    h, copies, probs, synd = u.inputs(case_id)
    assert h.shape == (c.m, c.n) and synd.shape == (c.rows, c.m)
    rank = u.gf2_rank(h)
    assert rank == min(c.m, c.n) - c.dup and c.n - rank == c.k and (rank < c.m) == bool(copies)
    assert all((h[a] != h[b]).nnz == 0 for a, b in copies)
    assert c.words == -(-(c.n + 1) // 64)
    deg = int(np.diff(h.indptr).max())
    assert deg == c.heavy if c.heavy else deg <= 6
    assert u.expected_kernel(c.m, c.n, deg, False, -1) == c.kernel0 and u.expected_kernel(c.m, c.n, deg, True, -1) == c.kernelw
    if c.group == "tall":
        assert c.mq == u.block_rows_per_thread(c.m) and (c.rows <= 8)
        assert u.expected_kernel(c.m, c.n, deg, True, 2).startswith("osd_big_kernel<")
    else:
        assert c.rows <= (48 if c.m < 128 else 24)


@pytest.mark.parametrize("case_id", IDS)
def test_case_shows_what_it_is_for(case_id, oracle_built):
    c = u.BY_ID[case_id]
    h, copies, probs, synd = u.inputs(case_id)
    dec0, _, conv = u.expected(case_id, u.OSD0, 0)
    assert (~conv).sum() >= (4 if c.group == "tall" else -(-c.rows // 3)), "too few rows reach OSD"
    solves = np.all((dec0.astype(np.int64) @ h.T.toarray().astype(np.int64)) % 2 == synd, axis=1)
    assert (~solves).any() == bool(copies), "a rank-deficient case carries rows outside the image of H, another case none"
    wt = np.log(1 / probs)
    for method, order in u.methods(c)[1:]:
        dec = u.expected(case_id, method, order)[0]
        won = (dec != dec0).any(axis=1)
        assert np.all((dec @ wt)[solves] <= (dec0 @ wt)[solves] + 1e-9)  # the sweep can only lower the weight (osd.hpp:177)
        if c.k == 0 or case_id in u.WITHOUT_A_WIN:
            assert not won.any()  # (k = 0: no candidate exists)
        else:
            assert won.any(), f"{method}/{order}: no row on which a candidate beats the OSD-0 solution"
    if c.group != "tall" and c.k >= 65 and case_id not in u.WITHOUT_A_WIN:
        d64, d70 = u.expected(case_id, u.OSD_CS, 64)[0], u.expected(case_id, u.OSD_CS, 70)[0]
        assert (d64 != d70).any(), "no row on which a pair reaching past column 63 wins"


def test_shapes_that_must_show_a_win():
    assert set(u.WITHOUT_A_WIN) <= {c.id for c in u.ALL_CASES if c.k > 0}
    assert "tall-2049x2200" not in u.WITHOUT_A_WIN
    assert any(c.mq and c.kernelw.startswith("osd_big_kernel") and c.id not in u.WITHOUT_A_WIN for c in u.TALL_CASES)


@pytest.mark.parametrize("case_id", IDS)
def test_oracle_equals_the_real_reference(case_id, oracle_built):
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference's headers)")
    c = u.BY_ID[case_id]
    h, copies, probs, synd = u.inputs(case_id)
    compared = 0
    for method, order in u.methods(c):
        if not u.reference_defined(c, method, order):
            continue
        ref = oracle.RefBpOsd(h, error_channel=probs, max_iter=c.max_iter, bp_method="minimum_sum", ms_scaling_factor=u.ALPHA, osd_method=method, osd_order=order)
        assert ref.k == c.k
        dec, _, it, conv = ref.decode_batch(synd, want_llr=False)
        want = u.expected(case_id, method, order)
        assert np.array_equal(dec, want[0]) and np.array_equal(it, want[1]) and np.array_equal(conv, want[2]), f"{method}/{order}"
        compared += 1
    assert compared >= 2  # (OSD-0 and OSD_E at the least)
