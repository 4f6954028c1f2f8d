"""The cases of tests/test_gpu_instantiations.py checked WITHOUT a GPU, from the builder (tests/ladder_util.py) and the oracle alone: every
matrix has the shape its case states, the rounds computed from its m by the size rules are the R in the kernel name the case expects, and its
syndromes make the decode do something -- some rows converge, some besides the two bad-byte rows do not."""
import re

import numpy as np
import pytest

import ladder_util as lu


def _ids(cases):
    return [c.id for c in cases]


def test_case_tables_have_the_stated_sizes():
    assert len(lu.EDGE_CASES) == 96 + 2 and len(lu.EDGE8_CASES) == 72 and len(lu.OUTSIDE_CASES) == 8
    assert len(set(_ids(lu.ALL_CASES))) == len(lu.ALL_CASES)
    # every selectable instantiation of the two lane = edge kernels is some case's kernel: 16 R x 3 forms, (10 + 8) R x 2 forms
    assert len({c.kernel for c in lu.EDGE_CASES}) == 48 and len({c.kernel for c in lu.EDGE8_CASES}) == 36
    assert set(lu.UNREACHABLE) <= set(_ids(lu.WAVE_CASES + lu.WAVE_PS_CASES))


@pytest.mark.parametrize("case", lu.ALL_CASES, ids=_ids(lu.ALL_CASES))
def test_builder_gives_the_stated_shape(case):
    h, probs, synd = lu.inputs(case.id)
    b = case.build
    rows, cols = np.asarray(h.sum(axis=1)).ravel(), np.asarray(h.sum(axis=0)).ravel()
    assert h.shape[0] == b["m"] and rows.max() == b["max_row"] and cols.max() == b["max_col"] and rows.min() == b.get("min_row", 1)
    assert (cols == 0).sum() == b.get("empty_cols", 0)
    if case.id.startswith("wave"):  # the wavefront ladders mix lighter nodes in: a weight-1 row (min_row) AND a weight-1 column
        assert rows.min() == 1 and cols[cols > 0].min() == 1
    if "base_row" in b:
        assert (rows > b["base_row"]).sum() == 1
    if "base_col" in b:
        assert (cols > b["base_col"]).sum() == 1
    assert synd.shape == (lu.BATCH, b["m"]) and not synd[0].any() and (synd[lu.BAD_ROWS[0]] == 2).sum() == 1 and (synd[lu.BAD_ROWS[1]] == 3).sum() == 1
    assert case.uniform == (len(set(probs.tolist())) == 1)
    if not case.uniform:
        assert (probs == 0.5).sum() == (0 if case.zero_prior is False else 1) and (probs == 0.7).sum() == 1


@pytest.mark.parametrize("case", lu.EDGE_CASES, ids=_ids(lu.EDGE_CASES))
def test_edge_rounds_and_form(case):
    h, _, _ = lu.inputs(case.id)
    r, uniform, noclamp = re.fullmatch(r"bp_edge_kernel<(\d+), (\w+), (\w+)>", case.kernel).groups()
    rows, cols = np.asarray(h.sum(axis=1)).ravel(), np.asarray(h.sum(axis=0)).ravel()
    assert lu.edge_rounds(h.shape[0]) == int(r) and rows.max() <= 4 and 1 <= cols.min() and cols.max() <= 2
    assert (uniform == "true") == case.uniform
    if noclamp == "true":  # the form without the clamp: no row lighter than 2, |alpha| <= 1
        assert rows.min() >= 2 and abs(case.alpha) <= 1 and not case.switches.get("EDGE_CLAMP")
    elif case.uniform:
        assert rows.min() == 1 or abs(case.alpha) > 1 or case.switches.get("EDGE_CLAMP")


@pytest.mark.parametrize("case", lu.EDGE8_CASES, ids=_ids(lu.EDGE8_CASES))
def test_edge8_rounds_and_form(case):
    h, _, _ = lu.inputs(case.id)
    r, dc, uniform = re.fullmatch(r"bp_edge8_kernel<(\d+), (\d), (\w+)>", case.kernel).groups()
    rows, cols = np.asarray(h.sum(axis=1)).ravel(), np.asarray(h.sum(axis=0)).ravel()
    assert rows.max() == 8 and cols.max() == int(dc) and cols.min() >= 1
    assert lu.edge8_rounds(h.shape[0], int(dc)) == int(r) and (uniform == "true") == case.uniform


def test_cases_just_outside_the_bounds_are_outside():
    by_id = {c.id: c for c in lu.OUTSIDE_CASES}
    shape = lambda i: lu.inputs(i)[0].shape
    assert lu.edge_rounds(shape("outside-m257")[0]) == 17
    assert lu.edge8_rounds(shape("outside-m97-dc3")[0], 3) == 0 and lu.edge8_rounds(shape("outside-m73-dc4")[0], 4) == 0
    for i in ("outside-weight5-row", "outside-weight3-column"):  # out of bp_edge_kernel's bounds, inside bp_edge8_kernel's: R from 8 lanes a row
        assert by_id[i].kernel == f"bp_edge8_kernel<{lu.edge8_rounds(shape(i)[0], 3)}, 3, true>"


@pytest.mark.parametrize("case", lu.ALL_CASES, ids=_ids(lu.ALL_CASES))
def test_oracle_converges_on_some_rows_and_not_on_others(case, oracle_built):
    conv = np.asarray(lu.expected(case.id)[3]).astype(bool)
    assert not conv[list(lu.BAD_ROWS)].any()
    others = np.delete(conv, lu.BAD_ROWS)
    assert others.any() and not others.all()
