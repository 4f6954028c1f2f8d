"""The cases of tests/relay_wave_util.py, checked on the CPU: each is outside both lane = edge ladders and on the rung of bp_wave_relay_kernel
it is named for, the restatement's output on it shows every kind of row the GPU comparison is about, and padding the strength tables as the
device does leaves the restatement's bits unchanged.  The size rules are restated in relay_wave_util.py; nothing is imported from the library's
dispatch."""
import numpy as np
import pytest

import mem_bp_util as mu
import relay_bp_util as ru
import relay_wave_util as wu


@pytest.mark.parametrize("name", list(wu.CASES))
def test_case_sits_on_its_rung_outside_the_edge_ladders(name):
    h = wu.matrix(name)
    rung = wu.CASES[name][0]
    assert not wu.edge_takes(h) and not wu.edge8_takes(h), f"{name}: a lane = edge kernel takes it"
    assert wu.wave_rung(h) == rung, f"{name}: lands on {wu.wave_rung(h)}, not {rung}"
    m, n = h.shape
    mp, np_ = (m + 63) // 64 * 64, (n + 63) // 64 * 64
    assert rung[0] * mp + 2 < 65536 and np_ + 1 < 65536, "16-bit positions"
    assert rung[0] * mp <= 2 * h.nnz + 1024, "the padding rule of the unforced plan"
    assert wu.wave_lds_bytes(h) <= 160 * 1024 - 64, "one syndrome fits LDS"
    assert np.bincount(h.indices, minlength=n).min() >= 1


def test_every_rung_has_a_case_and_the_sizes_differ():
    assert sorted({wu.CASES[k][0] for k in wu.CASES}) == sorted(wu.RUNGS)
    shapes = [wu.matrix(k).shape for k in wu.CASES]
    assert any(m % 64 for m, _ in shapes) and any(n % 64 for _, n in shapes) and any(n % 64 == 0 for _, n in shapes)
    assert any(np.diff(wu.matrix(k).indptr).min() < wu.CASES[k][0][0] for k in wu.CASES), "rows lighter than DR: phantom entries"
    assert any(np.bincount(wu.matrix(k).indices).min() < wu.CASES[k][0][1] for k in wu.CASES), "columns lighter than DC"


@pytest.mark.parametrize("name", list(wu.CASES))
def test_four_leg_batches_show_something(name):
    c = wu.case(name)
    assert c["synd"].shape[0] == 300 and tuple(c["leg_iters"]) == (8, 4, 4, 4) and c["stop_after"] == 2 and c["alpha"] == 0.625
    ru.assert_shows_something(wu.want(name), 2, f"{name}/300")
    b, want = wu.batch70(name)
    assert b["synd"].shape[0] == 70
    ru.assert_shows_something(want, 2, f"{name}/70")


@pytest.mark.parametrize("name", ["surface23", "hgp400"])
def test_six_leg_batches_show_a_replaced_solution(name):
    """surface23 is decoded in both forms on the GPU, and so is hgp400: a replaced solution in the one-wavefront and in the team form."""
    assert name in wu.SIX_LEGS
    c = wu.case(name, 6)
    assert tuple(c["leg_iters"]) == (12, 6, 6, 6, 6, 6) and c["stop_after"] == 3
    ru.assert_shows_something(wu.want(name, 6), 3, f"{name}/300, six legs", need_replaced=True)


def test_padded_tables_leave_the_bits_unchanged():
    """n = 200 (n % 64 = 8): the code with 56 isolated padding columns appended, a = 1.0 (p = 1 / (1 + e)) and gamma = 0 there -- what the
    device's padded tables hold -- decodes the real columns to the same bits, and the padding columns decide 0 with posterior 1.0."""
    import scipy.sparse as sp
    name = "ldpc200_36"
    b, want = wu.batch70(name)
    h = b["h"]
    n, np_ = h.shape[1], 256
    a = np.stack([mu.memory_a(b["probs"], g) for g in b["gamma"]])
    ap, gp = wu.padded_tables(a, b["gamma"], np_)
    assert ap.shape == gp.shape == (4, np_) and (ap[:, n:] == 1.0).all() and (gp[:, n:] == 0.0).all() and np.array_equal(ap[:, :n], a)
    hp = sp.hstack([h, sp.csr_matrix((h.shape[0], np_ - n), dtype=np.uint8)]).tocsr()
    pp = np.concatenate([b["probs"], np.full(np_ - n, 1.0 / (1.0 + np.e))])
    assert (np.log((1 - pp[n:]) / pp[n:]) == 1.0).all(), "the padding columns' prior is the padded a: 1.0"
    got = ru.relay_restatement(hp, pp, gp, b["leg_iters"], b["stop_after"], b["synd"], b["alpha"])
    assert np.array_equal(got[0][:, :n], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.array_equal(got[1][:, :n].view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64))
    assert not got[0][:, n:].any() and (got[1][:, n:] == 1.0).all()
