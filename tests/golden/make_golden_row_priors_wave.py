#!/usr/bin/env python3
"""Row-prior fixtures for codes of the lane = node kernel (bp_wave_rp_kernel), produced by the REFERENCE'S OWN classes.

Build container only.  The loop, the reference build (tests/golden/ref_python.py) and the fixture format are those of
tests/golden/make_golden_row_priors.py, whose ``run`` this script calls.  The files go to a directory of their own,
tests/golden/row_priors_wave/: tests/test_row_priors_api.py pins the list of files in tests/golden/row_priors/ name by name.
tests/row_priors_wave_util.py loads them with the loader of the others (``load_fixture``).

    python tests/golden/make_golden_row_priors_wave.py [--check]

* row_priors_hgp400_ms12_osd0     hypergraph_product_hx(regular_ldpc_code(16, 3, 4, seed=5)), 192 x 400, rung (8,4): min-sum 0.625, 12 iterations
                                  + OSD-0.  The probability level is chosen so that the reference leaves at least 10 rows to OSD; the count
                                  is printed.
* row_priors_ldpc128_ms_adaptive  regular_ldpc_code(128, 5, 16, seed=3), 40 x 128, rung (16,8): ms_scaling_factor = 0 (alpha = 1 - 2^-iteration),
                                  8 iterations; syndrome bytes 2 and 3; rows that stop early and rows that never converge.
Both: B = 70 (64 + 6), special probabilities in rows on both sides of row 64, one all-zero row.  Data only: the matrices come from
ldpc_amd.codes, the probabilities and syndromes from tests/row_priors_util.py.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_row_priors as base  # noqa: E402  (builds / loads the reference's package; reads --check)

from ldpc_amd.codes.synthetic import hypergraph_product_hx, regular_ldpc_code  # noqa: E402
from tests.row_priors_util import SPECIAL, draw_levels, levels_around, syndromes_of  # noqa: E402

base.ROW_PRIORS_DIR = os.path.join(HERE, "row_priors_wave")  # where ``run`` writes (and what ``--check`` reads)


def main():
    os.makedirs(base.ROW_PRIORS_DIR, exist_ok=True)
    # HGP [[400,16]] hx, min-sum: BP-12 + OSD-0 at rates where BP leaves rows to OSD
    h = hypergraph_product_hx(regular_ldpc_code(16, 3, 4, seed=5))
    rng = np.random.default_rng(707)
    levels = levels_around(0.03, count=11, spread=2.0)
    p_idx = draw_levels(rng, (70, h.shape[1]), levels, special_rows=(2, 41, 68))
    s = syndromes_of(h, np.clip(levels[p_idx], 0.0, 0.5), rng)
    s[4] = 0
    base.run("row_priors_hgp400_ms12_osd0", h, levels=levels, p_idx=p_idx, syndromes=s, own_p=0.03, max_iter=12, bp_method="minimum_sum",
             ms_scaling_factor=0.625, osd=True, min_unconverged=10,
             note="hypergraph_product_hx(regular_ldpc_code(16, 3, 4, seed=5)); decoding = BpOsdDecoder (OSD_0) output, the rest is BP's; "
                  "special probabilities " + repr(SPECIAL) + " in rows 2, 41, 68; row 4 all zero")
    # a (5,16)-regular LDPC code, rows of 16: the adaptive alpha
    h = regular_ldpc_code(128, 5, 16, seed=3)
    m, n = h.shape
    rng = np.random.default_rng(808)
    levels = levels_around(0.02, count=11, spread=4.0)
    p_idx = draw_levels(rng, (70, n), levels, special_rows=(3, 17, 40, 64, 69))
    s = syndromes_of(h, np.clip(levels[p_idx], 0.0, 0.5), rng)
    for b in range(70):  # every row but row 5 runs BP
        if not s[b].any():
            s[b, b % m] = 1
    s[5] = 0
    s[9, 0] = 2   # a byte > 1: never converges (bp.hpp:300)
    s[66, m - 1] = 3
    base.run("row_priors_ldpc128_ms_adaptive", h, levels=levels, p_idx=p_idx, syndromes=s, own_p=0.02, max_iter=8, bp_method="minimum_sum",
             ms_scaling_factor=0.0, want_mixed=True,
             note="regular_ldpc_code(128, 5, 16, seed=3), alpha = 1 - 2^-iteration; special probabilities " + repr(SPECIAL) +
                  " in rows 3, 17, 40, 64, 69; row 5 all zero; syndrome bytes 2 and 3 in rows 9 and 66")


if __name__ == "__main__":
    main()
