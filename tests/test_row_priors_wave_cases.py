"""Row priors on the codes of the lane = node kernel -- everything that needs no GPU (the GPU side: tests/test_gpu_row_priors_wave.py).

* every case of tests/row_priors_wave_util.py lands on its rung of bp_wave_rp_kernel and on no lane = edge plan, by the dispatch's rules
  restated (tests/relay_wave_util.py); ``hgp1600`` needs more than 150 KiB for one slot of the slot kernel, the other eight do not;
* the two fixtures of tests/golden/row_priors_wave/ (the reference's ``update_channel_probs`` + ``decode`` loop on HGP [[400,16]] with min-sum +
  OSD-0 and on a (5,16)-regular code with the adaptive alpha) hold what they were chosen for, and the per-row oracle reproduces them bit for bit;
* the oracle's answer on every case is one a wrong kernel cannot reproduce by accident: rows that converge early at several iteration counts,
  rows that run to max_iter, every special probability;
* the generator reproduces the committed fixtures wherever the reference is present (``--check``)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import relay_wave_util as wu
import row_priors_edge_util as eu
import row_priors_wave_util as ru
from row_priors_util import SPECIAL, llr_digest, ran_bp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_relay_kernels_eight_and_hgp1600():
    assert list(ru.CASES) == list(wu.CASES) + ["hgp1600"]
    assert sorted(set(ru.ADAPTIVE.values())) == sorted(wu.RUNGS), "alpha 0 once per rung"
    for name, rung in ru.ADAPTIVE.items():
        assert ru.CASES[name][0] == rung


@pytest.mark.parametrize("name", list(ru.CASES))
def test_case_lands_on_its_rung_and_on_no_edge_plan(name):
    h = ru.matrix(name)
    assert wu.wave_rung(h) == ru.CASES[name][0]
    assert not wu.edge_takes(h) and not wu.edge8_takes(h)
    m, n = h.shape
    mp, np_ = (m + 63) // 64 * 64, (n + 63) // 64 * 64
    assert ru.CASES[name][0][0] * mp + 2 < 65536 and np_ + 1 < 65536, "positions and column numbers are 16 bits (wave_pad)"
    assert ru.wave_rp_lds_bytes(h) <= 160 * 1024 - 64, "one syndrome fits LDS"
    assert h.nnz * 16 < (1 << 22), "onchip_bound"


def test_only_hgp1600_exceeds_one_slot():
    """small_lds_bytes(h, 1, rp) against the 150 KiB the slot kernel is given where another on-chip kernel takes the code's plain decode."""
    for name in ru.SLOT_CASES:
        b = ru.small_lds_bytes(ru.matrix(name))
        print(f"{name}: {b} B for one slot")
        assert b <= ru.SLOT_BUDGET
    assert 11_000 < min(ru.small_lds_bytes(ru.matrix(n)) for n in ru.SLOT_CASES) and max(ru.small_lds_bytes(ru.matrix(n)) for n in ru.SLOT_CASES) < 58_000
    h = ru.matrix("hgp1600")
    assert h.shape == (768, 1600) and h.nnz == 5376
    assert ru.small_lds_bytes(h) == 181328 > ru.SLOT_BUDGET
    assert ru.wave_rp_lds_bytes(h) == 88800


@pytest.mark.parametrize("name", list(ru.CASES))
def test_batch_of_the_case(name):
    c = ru.case(name)
    h, probs, synd = c["h"], c["probs"], c["synd"]
    assert probs.shape == (131, h.shape[1]) and synd.shape == (131, h.shape[0])
    assert ((probs >= 0) & (probs <= 1)).all()
    assert eu.distinct_rows(probs).all(), "every row has its own priors"
    assert sorted(np.flatnonzero(eu.has_special(probs)).tolist()) == sorted(ru.SPECIAL_ROWS)
    assert not synd[ru.ZERO_ROW].any()
    assert sorted(int(v) for v in np.unique(synd) if v > 1) == [2, 3] and synd[ru.BYTE2_ROW, 0] == 2 and synd[ru.BYTE3_ROW, -1] == 3
    assert not np.array_equal(probs[1], c["own"]), "the rows must not be the handle's own probabilities"


def _conditions(name, want, probs):
    dec, llr, it, cv = want
    early = cv & (it < ru.MAX_ITER)
    print(f"{name}: {int(early.sum())} rows converge before max_iter at {len(set(it[early].tolist()))} different counts "
          f"({int(it[early].min())} .. {int(it[early].max())}), {int((it == ru.MAX_ITER).sum())} run to {ru.MAX_ITER}")
    assert early.sum() >= 10 and len(set(it[early].tolist())) >= 3, "at least 10 rows that converge before max_iter, at three or more iteration counts"
    assert (it == ru.MAX_ITER).sum() >= 5, "at least 5 rows that run to max_iter"
    assert ru.special_kinds(probs) == set(SPECIAL), "a special row of each kind"
    assert not cv[[ru.BYTE2_ROW, ru.BYTE3_ROW]].any(), "a syndrome byte above 1 never converges (bp.hpp:300)"


@pytest.mark.parametrize("name", list(ru.CASES))
def test_oracle_answer_of_the_case(name):
    _conditions(name, ru.expected(name), ru.case(name)["probs"])


@pytest.mark.parametrize("name", list(ru.ADAPTIVE))
def test_oracle_answer_with_the_adaptive_factor(name):
    want = ru.expected(name, 0.0)
    _conditions(name + ", alpha 0", want, ru.case(name)["probs"])
    assert not oracle.bits_equal(want[1], ru.expected(name)[1]), "alpha 0 must not be alpha 0.625 again"


@pytest.mark.parametrize("name", ru.POOL_CASES)
def test_work_pool_batches(name):
    """20 011 rows by index: neighbours in the batch are 37 rows apart in the case, with different priors."""
    c = ru.case(name)
    idx = ru.pool_index(ru.BATCH)
    assert len(idx) == 20011 and (np.diff(idx) % ru.BATCH == 37).all() and set(idx.tolist()) == set(range(ru.BATCH))
    assert eu.distinct_rows(c["probs"]).all()
    assert ru.CASES[name][0] in ((8, 8), (4, 2))


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------------
def test_the_new_fixtures_are_there_and_small():
    got = sorted(f[:-4] for f in os.listdir(ru.WAVE_FIXTURE_DIR) if f.endswith(".npz"))
    assert got == sorted(ru.WAVE_FIXTURES)
    for name in ru.WAVE_FIXTURES:
        assert os.path.getsize(os.path.join(ru.WAVE_FIXTURE_DIR, name + ".npz")) < 64 * 1024


@pytest.mark.parametrize("name", ru.WAVE_FIXTURES)
def test_fixture_holds_what_it_was_chosen_for(name):
    c = ru.load_fixture(name)
    B, n = c["probs"].shape
    assert B == 70 and c["syndromes"].shape == (B, c["m"]) and c["bp_method"] == "minimum_sum"
    assert len({row.tobytes() for row in c["probs"]}) == B, "every row has its own priors"
    special = eu.has_special(c["probs"])
    assert special[:64].any() and special[64:].any(), "special probabilities in rows on both sides of row 64"
    for v in SPECIAL:
        assert (c["probs"] == v).any(), f"the special probability {v!r} never occurs"
    zero = ~ran_bp(c)
    assert zero.sum() == 1 and not c["decoding"][zero].any() and c["converge"][zero].all(), "one all-zero row, the reference's shortcut"
    ran = ran_bp(c)
    unconverged = int((~c["converge"][ran]).sum())
    early = int((c["converge"][ran] & (c["iterations"][ran] < c["max_iter"])).sum())
    print(f"{name}: {int(ran.sum())} rows ran BP, {early} stopped before max_iter, {unconverged} never converged")
    assert wu.wave_rung(c["h"]) == ru.FIXTURE_RUNG[name]
    if name == "row_priors_hgp400_ms12_osd0":
        assert c["osd"] and c["ms_scaling_factor"] == 0.625 and c["max_iter"] == 12 and (c["m"], c["n"]) == (192, 400)
        assert (c["h"] != ru.matrix("hgp400")).nnz == 0
        assert unconverged >= 10, "too few rows are left to OSD"
    else:
        assert not c["osd"] and c["ms_scaling_factor"] == 0.0 and c["max_iter"] == 8 and (c["m"], c["n"]) == (40, 128)
        assert (c["h"] != ru.matrix("ldpc128_516")).nnz == 0
        assert early > 0 and unconverged > 0, "rows that stop early AND rows that never converge"
        assert sorted(int(v) for v in np.unique(c["syndromes"]) if v > 1) == [2, 3], "syndrome bytes 2 and 3"
        assert not c["converge"][(c["syndromes"] > 1).any(axis=1)].any(), "a syndrome byte above 1 never converges (bp.hpp:300)"


@pytest.mark.parametrize("name", ru.WAVE_FIXTURES)
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


def test_the_older_fixtures_land_on_the_rungs_the_gpu_test_names():
    for name, rung in ru.OLDER_FIXTURES.items():
        c = ru.load_fixture(name)
        assert c["bp_method"] == "minimum_sum" and wu.wave_rung(c["h"]) == rung, name


@pytest.mark.skipif(not os.path.isdir("/root/reference/src_python/ldpc"), reason="the reference is not on this machine")
def test_generator_reproduces_the_fixtures():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_row_priors_wave.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("== committed fixture") == len(ru.WAVE_FIXTURES), r.stdout
