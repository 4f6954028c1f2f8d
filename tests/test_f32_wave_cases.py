"""The cases of tests/f32_wave_util.py, checked without a GPU: every builder gives the stated shape; the float32 restatement converges on
some rows and not on others, and never on the two rows with a syndrome byte above 1; the float32 and float64 restatements differ in the bit
pattern of at least one log-ratio, so a kernel that computed in FP64 (or a route that fell to an FP64 kernel) would be caught; and
ldpc_amd.bp_decoder.float32_lane_node_takes -- the planner's refusals restated in Python -- agrees with the case table."""
import numpy as np
import pytest
import scipy.sparse as sp

import f32_wave_util as wu
import ladder_util as lu

IDS = [c.id for c in wu.CASES]


def test_the_case_table():
    assert len(wu.CASES) == 14 and len(set(IDS)) == 14
    ladder = [c for c in wu.CASES if c.ladder]
    assert sorted((c.dr, c.dc, c.team) for c in ladder) == sorted((r, c, t) for r, c in wu.RUNGS for t in (False, True))
    assert all(c.mode == (5 if c.team else 4) for c in ladder)
    assert {wu.kernel_name(c.dr, c.dc, c.team) for c in wu.CASES} == {f"bp_wave_f32_kernel<{r}, {c}, {t}>" for r, c in wu.RUNGS for t in ("true", "false")}
    d = wu.BY_ID[wu.DEFAULT_MODE_CASE]
    assert d.mode == -1 and d.team and (d.dr, d.dc) == (16, 8)
    assert wu.route_name(True) == "bp_wave_team" and wu.route_name(False) == "bp_wave"


@pytest.mark.parametrize("case_id", IDS)
def test_the_builder_gives_the_stated_shape(case_id):
    c = wu.BY_ID[case_id]
    h, probs, synd = wu.inputs(case_id)
    h = sp.csr_matrix(h)
    m, n = h.shape
    rows, cols = np.diff(h.indptr), np.bincount(h.indices, minlength=n)
    assert int(rows.max()) == c.dr and int(cols.max()) == c.dc and wu.rung_of(int(rows.max()), int(cols.max())) == (c.dr, c.dc)
    assert int(rows.min()) >= 1 and int(cols.min()) >= 1
    want = (lu.ALL_CASES[[x.id for x in lu.ALL_CASES].index(c.ladder)].build if c.ladder else c.build)
    assert m == want["m"] and n == want["n"]
    assert synd.shape == (lu.BATCH, m) and synd.dtype == np.uint8 and len(probs) == n
    assert not synd[0].any() and int(synd[lu.BAD_ROWS[0]].max()) == 2 and int(synd[lu.BAD_ROWS[1]].max()) == 3
    if case_id == "wave_f32-4x2-n300-two-rounds-mode4":
        # U = 4 columns per lane (rows <= 4, columns <= 2): a wavefront's bit pass covers 256 columns a round
        assert (n + 63) // 64 * 64 == 320 and 256 < 320 <= 512


@pytest.mark.parametrize("case_id", IDS)
def test_the_restatement_on_the_case(case_id):
    dec, llr, it, cv = wu.expected(case_id)
    assert cv.any() and not cv.all(), f"{int(cv.sum())} of {len(cv)} rows converge"
    assert not cv[lu.BAD_ROWS[0]] and not cv[lu.BAD_ROWS[1]], "a syndrome byte above 1 never converges"
    assert (it[~cv] == lu.MAX_ITER).all() and it.min() >= 1
    assert np.array_equal(llr, llr.astype(np.float32).astype(np.float64), equal_nan=True)
    llr64 = wu.expected(case_id, np.float64)[1]
    differ = int(np.count_nonzero(llr.view(np.uint64) != llr64.view(np.uint64)))
    assert differ > 0, "float32 and float64 give the same log-ratio bits: the case cannot tell the two arithmetics apart"


@pytest.mark.parametrize("case_id", IDS)
def test_float32_lane_node_takes_the_case(case_id):
    from ldpc_amd.bp_decoder import float32_lane_node_takes
    h = wu.inputs(case_id)[0]
    assert float32_lane_node_takes(h) and float32_lane_node_takes(h, forced=True)


def _band(m, w, n=None):
    """m rows of w entries: row i takes columns i w .. i w + w - 1, modulo n (default m w: every column has one entry)."""
    n = m * w if n is None else n
    i = np.arange(m)
    cols = (i[:, None] * w + np.arange(w)[None, :]) % n
    return sp.csr_matrix((np.ones(m * w, np.uint8), (np.repeat(i, w), cols.ravel())), shape=(m, n))


def test_float32_lane_node_takes_restates_the_refusals():
    from ldpc_amd.bp_decoder import float32_lane_node_takes as takes
    assert takes(_band(40, 16)) and not takes(_band(40, 17)), "rows of 17"
    col8 = sp.csr_matrix(np.vstack([np.ones((8, 1), np.uint8), np.zeros((4, 1), np.uint8)]))
    col9 = sp.csr_matrix(np.vstack([np.ones((9, 1), np.uint8), np.zeros((3, 1), np.uint8)]))
    wide = sp.hstack([sp.identity(12, dtype=np.uint8, format="csr")] * 3, format="csr")
    assert takes(sp.hstack([col8, wide], format="csr")) and not takes(sp.hstack([col9, wide], format="csr")), "a column of 9"
    # 16-bit column numbers: np + 1 < 65536, so n <= 65 472; two entries a row keep the rows' rules satisfied
    i = np.arange(1000)
    two = lambda n: sp.csr_matrix((np.ones(2000, np.uint8), (np.repeat(i, 2), np.stack([i, n - 1 - i], axis=1).ravel())), shape=(1000, n))  # noqa: E731
    assert not takes(two(65473), forced=True), "n overflows the u16 tables"
    # ... and with n inside the tables such a code fails on LDS: its position table alone, 2 x 65 472 x 2 bytes, is more than 160 KiB
    assert not takes(two(65472), forced=True)
    assert takes(two(20000))
    # padding: one row of 16 beside 900 rows of one entry pads 16 x 960 slots for 916 entries -- refused by default, taken when forced
    lop = sp.vstack([sp.csr_matrix(np.r_[np.ones(16, np.uint8), np.zeros(884, np.uint8)][None, :]), sp.identity(900, dtype=np.uint8, format="csr")], format="csr")
    assert not takes(lop) and takes(lop, forced=True)
    # 16-bit positions: DR * mp + 2 < 65536 -- 4096 rows of 16 over 8192 columns of 8
    big = _band(4096, 16, 8192)
    assert int(np.bincount(big.indices).max()) == 8 and not takes(big, forced=True)
    assert not takes(sp.csr_matrix((3, 5), dtype=np.uint8))


def test_the_python_allowance_is_the_headers():
    """float32_lane_node_takes restates WAVE_F32_LDS_STATIC and the LDS sizes of bp_wave_f32_kernel.h."""
    import os
    import re
    from ldpc_amd.bp_decoder import _bp_decoder as bd
    text = open(os.path.join(os.path.dirname(os.path.abspath(bd.__file__)), "..", "csrc", "bp_wave_f32_kernel.h")).read()
    assert int(re.search(r"constexpr size_t WAVE_F32_LDS_STATIC = (\d+);", text).group(1)) == bd._WAVE_F32_LDS_STATIC
    shared_vars = re.findall(r"^    __shared__ (.+);$", text, re.M)
    assert shared_vars == ["int team_unsat[2]", "long long team_b", "unsigned long long clk_stamp[2]"]
    assert 2 * 4 + 8 + 2 * 8 <= bd._WAVE_F32_LDS_STATIC
    assert "(size_t)DR * mp * 2 + (size_t)DC * np * 2 + (size_t)mp;" in text
    assert "((size_t)DR * mp + 2) * 4 + (want_llr ? (size_t)np * 4 : 0) + (size_t)(np / 64 + 1) * 8 + (size_t)mp;" in text
    assert bd._WAVE_RUNGS == wu.RUNGS
