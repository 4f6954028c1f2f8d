"""Row priors on the codes of the lane = edge kernels -- everything that needs no GPU (the GPU side: tests/test_gpu_row_priors_edge.py).

* the two fixtures of tests/golden/row_priors_edge/ (the reference's ``update_channel_probs`` + ``decode`` loop on BB [[144,12,12]] with
  min-sum + OSD-0 and on a rotated surface code with the adaptive alpha) hold what they were chosen for, and the per-row oracle reproduces
  them bit for bit;
* the cases the GPU tests run name every instantiation of bp_edge_rp_kernel and bp_edge8_rp_kernel, and their batches have, in both full
  tiles of 64 rows and in the 3-row tail, rows with special probabilities and rows whose priors no other row has;
* the generator reproduces the committed fixtures wherever the reference is present (``--check``)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ladder_util as lu
import oracle
import row_priors_edge_util as ru
from row_priors_util import SPECIAL, llr_digest, ran_bp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_fixtures_are_there_and_small():
    got = sorted(f[:-4] for f in os.listdir(ru.EDGE_FIXTURE_DIR) if f.endswith(".npz"))
    assert got == sorted(ru.EDGE_FIXTURES)
    for name in ru.EDGE_FIXTURES:
        assert os.path.getsize(os.path.join(ru.EDGE_FIXTURE_DIR, name + ".npz")) < 64 * 1024


@pytest.mark.parametrize("name", ru.EDGE_FIXTURES)
def test_fixture_holds_what_it_was_chosen_for(name):
    c = ru.load_fixture(name)
    B, n = c["probs"].shape
    assert B == 70 and c["syndromes"].shape == (B, c["m"]) and c["bp_method"] == "minimum_sum"
    assert len({row.tobytes() for row in c["probs"]}) == B, "every row has its own priors"
    special = ru.has_special(c["probs"])
    assert special[:64].any() and special[64:].any(), "special probabilities in rows of both tiles"
    for v in SPECIAL:
        assert (c["probs"] == v).any(), f"the special probability {v!r} never occurs"
    zero = ~ran_bp(c)
    assert zero.sum() == 1 and not c["decoding"][zero].any() and c["converge"][zero].all(), "one all-zero row, the reference's shortcut"
    ran = ran_bp(c)
    unconverged = int((~c["converge"][ran]).sum())
    early = int((c["converge"][ran] & (c["iterations"][ran] < c["max_iter"])).sum())
    print(f"{name}: {int(ran.sum())} rows ran BP, {early} stopped before max_iter, {unconverged} never converged")
    if name == "row_priors_bb144_ms10_osd0":
        assert c["osd"] and c["ms_scaling_factor"] == 0.625 and c["max_iter"] == 10 and (c["m"], c["n"]) == (72, 144)
        assert unconverged >= 10, "too few rows are left to OSD"
    else:
        assert not c["osd"] and c["ms_scaling_factor"] == 0.0 and (c["m"], c["n"]) == (12, 25)
        assert early > 0 and unconverged > 0, "rows that stop early AND rows that never converge"
        assert sorted(int(v) for v in np.unique(c["syndromes"]) if v > 1) == [2, 3], "syndrome bytes 2 and 3"
        assert not c["converge"][(c["syndromes"] > 1).any(axis=1)].any(), "a syndrome byte above 1 never converges (bp.hpp:300)"


@pytest.mark.parametrize("name", ru.EDGE_FIXTURES)
def test_fixture_equals_the_oracle_row_by_row(name):
    c = ru.load_fixture(name)
    B, n = c["probs"].shape
    llr = np.zeros((B, n))
    with np.errstate(all="ignore"):
        for b in np.flatnonzero(ran_bp(c)):
            o = oracle.BpOracle(c["h"], error_channel=c["probs"][b], max_iter=c["max_iter"], bp_method=c["bp_method"],
                                ms_scaling_factor=c["ms_scaling_factor"])
            dec, l, it, cv = o.decode_batch(c["syndromes"][b:b + 1])
            llr[b] = l[0]
            assert bool(cv[0]) == bool(c["converge"][b]) and int(it[0]) == int(c["iterations"][b]), f"row {b}"
            want = dec[0] if (cv[0] or not c["osd"]) else o.osd0(c["syndromes"][b], l[0])
            assert np.array_equal(want, c["decoding"][b]), f"row {b}: decisions"
    k = len(c["llr"])
    assert oracle.bits_equal(llr[:k], c["llr"]), "log-ratios of the rows stored in full"
    assert np.array_equal(llr_digest(llr), c["llr_crc"]), "log-ratio bit patterns, every row"


def test_the_fixtures_codes_take_the_kernels_the_gpu_test_names():
    """plan_edge: rows <= 4, columns <= 2, ceil(4 m / 64) rounds; plan_edge8: rows <= 8, columns <= 3 -> DC 3, the smallest compiled R >= ceil(8 m / 64)."""
    c = ru.load_fixture("row_priors_surface_ms_adaptive")
    assert np.diff(c["h"].indptr).max() <= 4 and np.diff(c["h"].tocsc().indptr).max() <= 2 and np.diff(c["h"].tocsc().indptr).min() >= 1
    assert lu.edge_rounds(c["m"]) == 1
    c = ru.load_fixture("row_priors_bb144_ms10_osd0")
    assert np.diff(c["h"].indptr).max() == 6 and np.diff(c["h"].tocsc().indptr).max() == 3
    assert lu.edge8_rounds(c["m"], 3) == 9


def test_one_case_per_instantiation():
    """16 bp_edge_rp_kernel<R>, and one bp_edge8_rp_kernel<R, DC> per (R, DC) plan_edge8 can return."""
    names = [ru.rp_kernel_name(c.kernel) for c in ru.CASES]
    want = [f"bp_edge_rp_kernel<{r}>" for r in range(1, 17)] + [f"bp_edge8_rp_kernel<{r}, {dc}>" for dc in (3, 4) for r in lu.EDGE8_ROUNDS[dc]]
    assert sorted(names) == sorted(want) and len(set(names)) == 34
    for c in ru.CASES:
        assert not c.uniform and c.method == "minimum_sum" and c.mode == 6
        others = [o for o in lu.EDGE_CASES + lu.EDGE8_CASES if o.kernel == c.kernel]
        assert c.build["m"] == min(o.build["m"] for o in others), "the smallest code of its instantiation"


@pytest.mark.parametrize("case", ru.CASES, ids=[c.id for c in ru.CASES])
def test_batches_of_the_gpu_cases(case):
    h, own, synd = lu.inputs(case.id)
    probs = ru.row_probs(case.id)
    assert probs.shape == (lu.BATCH, h.shape[1]) == (131, h.shape[1]) and synd.shape[0] == 131
    assert ((probs >= 0) & (probs <= 1)).all()
    distinct, special = ru.distinct_rows(probs), ru.has_special(probs)
    for lo, hi in ((0, 64), (64, 128), (128, 131)):
        assert distinct[lo:hi].any(), f"rows {lo} .. {hi - 1}: no row whose priors differ from every other row's"
        assert special[lo:hi].any(), f"rows {lo} .. {hi - 1}: no row with special probabilities"
    assert not np.array_equal(probs[0], own), "the rows must not be the handle's own probabilities"


@pytest.mark.parametrize("key", list(ru.POOL_CASES))
def test_work_pool_batches(key):
    """20 011 rows by index: neighbours in the batch have different priors, and the expectation holds nothing the poison could pass for."""
    h, own, synd, probs, max_iter, alpha, want, kernel = ru.pool_inputs(key)
    assert ru.distinct_rows(probs).all() and not ru.has_special(probs).any()
    idx = ru.pool_index(len(synd))
    assert len(idx) == 20011 and (np.diff(idx) % len(synd) == 37 % len(synd)).all()
    assert not np.isnan(want[1]).any() and want[2].min() >= 1
    assert want[3].any() and not want[3].all(), "rows that converge and rows that do not"
    assert kernel in ("bp_edge_rp_kernel<1>", "bp_edge8_rp_kernel<9, 3>")


@pytest.mark.skipif(not os.path.isdir("/root/reference/src_python/ldpc"), reason="the reference is not on this machine")
def test_generator_reproduces_the_fixtures():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_row_priors_edge.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("== committed fixture") == len(ru.EDGE_FIXTURES), r.stdout
