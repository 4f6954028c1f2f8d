"""The cases of tests/bpgd_wave_util.py, on the CPU: each shows, on the NumPy restatement's own output, what the GPU test
(tests/test_gpu_bpgd_wave.py) is there to compare -- and the switch, the keywords and ``lane_node_takes`` as far as they need no GPU."""
import numpy as np
import pytest

import bpgd_util as gu
import bpgd_wave_util as gw
import f32_util as fu
import ladder_util as lu
import relay_wave_util as wu


@pytest.mark.parametrize("name", list(wu.CASES))
def test_every_case_shows_all_three_kinds_of_row(name):
    c, want = gw.every_instantiation(name), gw.want_instantiation(name)
    assert c["synd"].shape[0] == 70 and (c["round_iters"], c["max_rounds"], c["freeze_llr"], c["alpha"]) == (3, 6, 25.0, 0.625)
    early, late, never = gu.shows(want, gw.R)
    print(f"{name}: {early} rows solved in round 0, {late} after a decimation, {never} never")
    assert early > 0 and late > 0 and never > 0
    assert (early, late, never) == gw.SHOWS[name]
    hd = c["h"].toarray().astype(np.int64)
    ok = np.flatnonzero(want[3])
    assert np.array_equal((want[0][ok].astype(np.int64) @ hd.T) & 1, c["synd"][ok]), "a converged row reproduces its syndrome"
    assert (want[2][~want[3]] == gw.T * gw.R).all()


def test_the_cases_lie_outside_both_lane_edge_ladders_and_on_every_rung():
    from ldpc_amd.bpgd_decoder import lane_edge_route, lane_node_takes
    assert sorted({wu.CASES[name][0] for name in wu.CASES}) == sorted(wu.RUNGS)
    for name in wu.CASES:
        h = wu.matrix(name)
        assert not wu.edge_takes(h) and not wu.edge8_takes(h) and wu.wave_rung(h) == wu.CASES[name][0], name
        assert lane_edge_route(h) == "unavailable" and lane_node_takes(h), name


def test_the_pool_batch_mixes_the_kinds_of_row():
    """300 rows of ldpc64_58 tiled to 20 011: a row solved in round 0 follows a row that froze five columns, a walker follows a row solved
    late, and neighbouring rows freeze different columns -- a wavefront that kept its predecessor's masks, messages or posteriors decodes other bits."""
    c, want = gw.tiled("ldpc64_58", gw.POOL_ROWS)
    assert c["synd"].shape[0] == gw.POOL_ROWS and np.array_equal(c["synd"][300:600], c["synd"][:300])
    sr, chosen = want[4]["solved_round"], want[4]["frozen"]
    assert gu.shows(gw.want_all_rows("ldpc64_58"), gw.R) == (133, 93, 74)
    assert len(np.flatnonzero(~want[3][:-1] & (sr[1:] == 0))) and len(np.flatnonzero((sr[:-1] > 0) & ~want[3][1:]))
    assert (chosen[:-1, 0] != chosen[1:, 0]).any()
    assert not np.isnan(want[1]).any() and want[2].min() >= 1, "the poison of the outputs differs from every expected value"
    early, late, never = gu.shows(gw.want_all_rows("hgp400"), gw.R)
    assert early > 0 and late > 0 and never > 0


def test_ties():
    c = gw.tie_case()
    assert c["h"].shape == (257, 258) and not wu.edge_takes(c["h"]) and not wu.edge8_takes(c["h"]) and wu.wave_rung(c["h"]) == (4, 2)
    want = gu.expected("wave_gd|tie", c)
    assert not want[3].any() and (want[2] == 12).all()
    assert want[4]["frozen"].tolist() == [[2, 0, 1, 3, 4]] * 3
    # the first choice's key is shared by at least two eligible columns: the posteriors after round 0 are a plain decode's after T iterations
    plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], c["round_iters"], c["alpha"], np.float64)
    for b in range(3):
        key = np.abs(plain[1][b])
        assert np.count_nonzero(key == key.max()) >= 2 and int(np.argmax(key)) == 2, f"row {b}"


def test_nothing_left_to_freeze():
    c = gw.all_frozen_case()
    want = gu.expected("wave_gd|all_frozen", c)
    f = want[4]["frozen"]
    assert f.shape == (3, 66) and (f[:, :64] >= 0).all() and (f[:, 64:] == -1).all()
    assert all(sorted(row[:64].tolist()) == list(range(64)) for row in f), "every column is frozen once"
    assert (want[2] == 67).all() and not want[3].any()


@pytest.mark.parametrize("alpha,freeze", gw.SPECIAL)
def test_special_priors(alpha, freeze):
    c = gw.special_priors_case(alpha, freeze)
    want = gu.expected(f"wave_gd|special|{alpha}|{freeze}", c)
    early, late, never = gu.shows(want, c["max_rounds"])
    print(f"special priors, alpha {alpha}, C = {freeze}: {early}, {late}, {never}")
    assert want[3].any(), "some row converges"
    f = want[4]["frozen"]
    assert (f >= 0).any(), "some row decimates"
    infinite = [j for j, p in gw.SPECIAL_COLUMNS.items() if p in (0.0, 1.0)]
    assert len(infinite) == 4 and not np.isin(f, infinite).any(), "a column with p = 0 or 1 is never chosen"


def test_an_empty_column():
    c = gw.empty_column_case()
    cols = np.bincount(c["h"].indices, minlength=c["h"].shape[1])
    from ldpc_amd.bpgd_decoder import lane_edge_route, lane_node_takes
    assert cols.min() == 0 and lane_edge_route(c["h"]) == "unavailable" and lane_node_takes(c["h"])
    want = gu.expected("wave_gd|empty_column", c)
    early, late, never = gu.shows(want, gw.R)
    print(f"outside-empty-column at rate {gw.EMPTY_COLUMN_RATE}: {early}, {late}, {never}")
    assert (want[4]["frozen"] >= 0).any(), "a decimation happens"
    assert want[3].any() and not want[3].all()


def test_one_round_is_the_plain_decode():
    c = gw.one_round_case()
    want = gu.expected("wave_gd|one_round", c)
    plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], c["round_iters"], c["alpha"], np.float64)
    assert plain[3].any() and not plain[3].all()
    assert np.array_equal(want[0], plain[0]) and np.array_equal(want[2], plain[2]) and np.array_equal(want[3], plain[3])
    assert np.array_equal(want[1].view(np.uint64), np.ascontiguousarray(plain[1]).view(np.uint64))


# ---- the switch, without a GPU ---------------------------------------------------------------------------------------------------------------
def test_lane_node_takes_restates_the_size_rules():
    from ldpc_amd.bpgd_decoder import lane_node_takes
    assert not lane_node_takes(fu.irregular_case()["h"]), "columns of 11"
    assert not lane_node_takes(fu.heavy_rows_case()["h"]), "rows of 20"
    for case in lu.OUTSIDE_CASES:  # (small codes with rows of at most 9 and columns of at most 5 entries)
        h = lu.inputs(case.id)[0]
        assert lane_node_takes(h) == (wu.wave_rung(h) is not None and wu.wave_rung(h)[0] * ((h.shape[0] + 63) // 64 * 64) <= 2 * h.nnz + 1024), case.id
    # the LDS sizes: bb144 x 12 rounds (864 x 2520, rung (8,4)) needs 35 712 shared + 79 728 private bytes
    mp, np_ = 896, 2560
    up16 = lambda b: (b + 15) & ~15  # noqa: E731
    assert up16(8 * mp * 2 + 4 * np_ * 2 + mp) == 35712 and up16((8 * mp + 2) * 8 + np_ * 8 + 3 * (np_ // 64 + 1) * 8 + mp) == 79728


def _two_per_row(m, n):
    """m rows of two entries over n columns (row i: columns i % n and (i + 1) % n): rung (4,2) for m <= n."""
    import scipy.sparse as sp
    i = np.arange(m)
    return sp.csr_matrix((np.ones(2 * m, np.uint8), (np.repeat(i, 2), np.stack([i % n, (i + 1) % n], axis=1).ravel())), shape=(m, n))


def test_the_lds_budget_leaves_room_for_the_kernels_static_lds():
    """The team forms of bp_wave_gd_kernel hold 224 bytes of static LDS (two flags, the team's syndrome number, sixteen winners of 8 + 4
    bytes, the clock stamps); plan_wave_gd and lane_node_takes hand out 160 KiB less WAVE_GD_LDS_STATIC, so dynamic + static LDS never exceeds
    the 163 840 bytes a workgroup has.  A code whose dynamic part alone is 163 776 bytes (it would need 164 000) is not taken."""
    import os
    import re
    from ldpc_amd.bpgd_decoder import _bpgd_decoder as bd
    csrc = os.path.join(os.path.dirname(os.path.abspath(bd.__file__)), "..", "csrc")
    text = open(os.path.join(csrc, "bp_wave_gd_kernel.h")).read()
    allowance = int(re.search(r"constexpr size_t WAVE_GD_LDS_STATIC = (\d+);", text).group(1))
    assert allowance == bd._WAVE_GD_LDS_STATIC, "lane_node_takes restates the kernel header's allowance"
    maxw = int(re.search(r"constexpr int MAXW = (\d+);", text).group(1))
    shared_vars = re.findall(r"^    __shared__ (.+);$", text, re.M)
    assert shared_vars == ["int team_unsat[2]", "long long team_b", "double team_key[MAXW]", "int team_tag[MAXW]", "unsigned long long clk_stamp[2]"]
    static = 2 * 4 + 8 + maxw * 8 + maxw * 4 + 2 * 8
    assert static == 224 and static <= allowance
    assert "static_assert(sizeof(team_unsat) + sizeof(team_b) + sizeof(team_key) + sizeof(team_tag) + sizeof(clk_stamp) <= WAVE_GD_LDS_STATIC" in text
    assert "WAVE_GD_LDS_STATIC);" in open(os.path.join(csrc, "host_onchip.h")).read(), "plan_wave_gd reserves it"
    up16 = lambda b: (b + 15) & ~15  # noqa: E731

    def dynamic(mp, np_):  # rung (4,2): the shared tables + one syndrome's private region
        return up16(4 * mp * 2 + 2 * np_ * 2 + mp) + up16((4 * mp + 2) * 8 + np_ * 8 + 3 * (np_ // 64 + 1) * 8 + mp)
    # the reviewer's example: 2817 <= m <= 2880, 3393 <= n <= 3456 -- 163 776 bytes, within 160 KiB - 64 but not with the static 224 on top
    assert dynamic(2880, 3456) == 163776 and 163776 + static > 160 * 1024
    for m, n in ((2880, 3456), (2817, 3393)):
        assert not bd.lane_node_takes(_two_per_row(m, n)), (m, n)
    # the largest (mp, np) of that shape that fits with the allowance is taken, and fits with the real static part too
    assert dynamic(2880, 3392) <= 160 * 1024 - allowance and dynamic(2880, 3392) + static <= 160 * 1024
    assert bd.lane_node_takes(_two_per_row(2880, 3392))
    # no padded size the rule takes overflows the workgroup's LDS, on any rung
    for dr, dc in bd._WAVE_RUNGS:
        for mp in range(64, 8192, 64):
            lo = up16(dr * mp * 2 + mp) + up16((dr * mp + 2) * 8 + mp)
            if lo > 160 * 1024:
                break
            for np_ in range(64, 16384, 64):
                d = up16(dr * mp * 2 + dc * np_ * 2 + mp) + up16((dr * mp + 2) * 8 + np_ * 8 + 3 * (np_ // 64 + 1) * 8 + mp)
                if d > 160 * 1024 - allowance:
                    break
                assert d + static <= 160 * 1024


def test_the_keywords_and_the_refusals_before_a_handle_exists():
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.bpgd_decoder import BpgdDecoder
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    h = wu.matrix("ldpc64_58")
    d = BpgdDecoder(h, error_rate=0.05)
    assert d.decimation_lane_node is False and d.route == "unavailable"
    with pytest.raises(NotImplementedError, match="neither lane = edge kernel family takes this code.*the lane = node route for larger codes and a per-pass route are not built yet"):
        d.decode(np.zeros(h.shape[0], np.uint8) + np.eye(1, h.shape[0], 0, dtype=np.uint8)[0])
    assert BpgdDecoder(h, error_rate=0.05, lane_node=True).decimation_lane_node is True
    with pytest.raises(ValueError, match="decimation_lane_node must be a bool"):
        BpgdDecoder(h, error_rate=0.05, lane_node=1)
    # a code neither the lane = edge families nor the lane = node kernel take: refused before a handle exists, with the new sentence
    big = fu.irregular_case()
    d = BpgdDecoder(big["h"], error_rate=0.05, lane_node=True)
    assert d.route == "unavailable"
    with pytest.raises(NotImplementedError, match="neither lane = edge kernel family nor the lane = node kernel takes this code.*a per-pass route is not built"):
        d.decode_batch(big["synd"])
    b = BpDecoder(h, error_rate=0.05, max_iter=4, bp_method="minimum_sum", input_vector_type="syndrome")
    assert b.decimation_lane_node is False
    b.decimation_lane_node = True
    assert b.decimation_lane_node is True and b.decimation is None
    from test_dem_sampler_twin import dem_models
    model = dem_models()["bb144x3"]
    assert MonteCarloDemSimulation(model, target_run_count=64, decimation=dict(round_iters=3, max_rounds=6)).decimation_lane_node is False
    assert MonteCarloDemSimulation(model, target_run_count=64, decimation=dict(round_iters=3, max_rounds=6), decimation_lane_node=True).decimation_lane_node is True
    with pytest.raises(ValueError, match="decimation_lane_node"):
        MonteCarloDemSimulation(model, target_run_count=64, decimation_lane_node="yes")
