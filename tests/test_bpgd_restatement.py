"""BP with guided decimation without a GPU: the NumPy restatement (tests/bpgd_util.py) against the plain restatement where it must equal it,
what it buys on the BB [[144,12,12]] batch, ties, "nothing left to freeze", the infinite priors, freeze_llr = inf -- and the argument
errors and refusals of the Python layer, each before any handle exists."""
import numpy as np
import pytest

import bpgd_util as gu
import f32_util as fu
from oracle import bits_equal


def _equal(got, want, what):
    for k, name in ((0, "decoding"), (2, "iterations"), (3, "converge")):
        assert np.array_equal(got[k], want[k]), f"{what}: {name}"
    assert bits_equal(got[1], want[1]), f"{what}: log-ratios differ in some bit"


def _reproduces(case, out):
    hd = case["h"].toarray().astype(np.int64)
    rows = np.flatnonzero(out[3])
    return np.array_equal((out[0][rows].astype(np.int64) @ hd.T) & 1, case["synd"][rows])


# ---- the invariants -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["hamming3", "rep5", "bb144"])
def test_one_round_is_the_plain_decode(key):
    """R = 1 is the plain FP64 decode with max_iter = T, bit for bit: decisions, posterior bits, counts, flags."""
    c = {"hamming3": lambda: fu.small_case("hamming3", 0.625), "rep5": lambda: fu.small_case("rep5", 0.0), "bb144": fu.bb144_case}[key]()
    want = fu.expected(f"bpgd|{key}", c, np.float64)
    assert want[3].any() and not want[3].all()
    for freeze in (25.0, np.inf):
        _equal(gu.bpgd_restatement(c["h"], c["probs"], c["synd"], c["max_iter"], 1, freeze, c["alpha"]), want, f"{key}, C = {freeze}")


def test_bb144_solves_more_rows_than_plain_min_sum_with_the_same_budget():
    """bb144_case() (70 rows, p = 0.06, alpha 0.625), T = 5, R = 144, C = 25 against plain min-sum with max_iter = 720: 67 against 52 rows,
    15 only BPGD solves, none only plain solves; R = 16: 53."""
    c = fu.bb144_case()
    case = dict(c, round_iters=5, max_rounds=144, freeze_llr=25.0)
    got = gu.expected("bb144|5x144", case)
    plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], 720, c["alpha"], np.float64)
    solved, plain_solved = int(got[3].sum()), int(plain[3].sum())
    only_gd, only_plain = int((got[3] & ~plain[3]).sum()), int((plain[3] & ~got[3]).sum())
    print(f"BPGD solves {solved} rows, plain min-sum 720 {plain_solved}; {only_gd} only BPGD, {only_plain} only plain; {gu.shows(got, 144)}")
    assert solved > plain_solved, "BPGD solves no more rows than plain min-sum with the same budget"
    assert only_plain == 0, "a row plain min-sum solves is lost"
    assert _reproduces(case, got), "a converged row does not reproduce its syndrome"
    assert (solved, plain_solved, only_gd, only_plain) == (67, 52, 15, 0)
    early, late, never = gu.shows(got, 144)
    assert early > 0 and late > 0 and never > 0
    assert (got[2][~got[3]] == 720).all() and (got[2][got[3]] < 720).all()
    # a row solved after a decimation froze a column in every round before that, none after
    d = got[4]
    b = int(np.flatnonzero(d["solved_round"] > 0)[0])
    r = int(d["solved_round"][b])
    assert (d["frozen"][b, :r] >= 0).all() and (d["frozen"][b, r:] == -1).all() and len(set(d["frozen"][b, :r])) == r
    assert int(gu.bpgd_restatement(c["h"], c["probs"], c["synd"], 5, 16, 25.0, c["alpha"])[3].sum()) == 53


# ---- ties, nothing left to freeze, infinite priors, an infinite freeze_llr -------------------------------------------------------------------------------
def test_ties_take_the_smallest_column_and_all_frozen_rounds_still_run():
    c = gu.tie_case()
    n = c["h"].shape[1]
    assert c["max_rounds"] == n + 2 and (c["synd"] > 1).any(axis=1).all()
    got = gu.expected("tie", c)
    assert not got[3].any() and (got[2] == c["max_rounds"] * c["round_iters"]).all(), "a syndrome byte > 1 never converges: every round runs"
    for b in (0, 1):
        assert got[4]["frozen"][b].tolist() == list(range(n)) + [-1], f"row {b}: ties go to the smallest column, then nothing is left"
    assert sorted(got[4]["frozen"][2][:n].tolist()) == list(range(n)) and got[4]["frozen"][2][n] == -1
    assert got[4]["frozen"][2].tolist() != got[4]["frozen"][0].tolist()
    assert np.isinf(got[1][:2]).all(), "every column frozen at +-inf: the posteriors are infinite"


@pytest.mark.parametrize("code,alpha", [("hamming3", 0.625), ("rep5", 0.0)])
def test_infinite_priors_are_never_chosen(code, alpha):
    """_edge_channel: p = 0, 1, 0.5, 1e-300 -- the columns with p = 0 and p = 1 (infinite log-ratios) are frozen from the start."""
    c = gu.edge_channel_case(code, alpha)
    infinite = np.flatnonzero(~np.isfinite(fu.priors_f64(c["probs"])))
    assert len(infinite) == 2 and set(c["probs"][infinite]) == {0.0, 1.0}
    got = gu.expected(f"edge_channel|{code}", c)
    chosen = got[4]["frozen"]
    assert (chosen >= 0).any() and not np.isin(chosen, infinite).any()
    walked = np.flatnonzero(~got[3])
    assert len(walked) and got[3].any()
    finite = c["h"].shape[1] - 2
    for b in walked:
        picks = chosen[b][chosen[b] >= 0]
        assert len(set(picks)) == len(picks) <= finite, "a column is frozen once"
    assert any((chosen[b] >= 0).sum() == finite and chosen[b][-1] == -1 for b in walked), "no row freezes every finite column and runs on"
    assert _reproduces(c, got)


def test_freeze_llr_inf_runs_and_its_nans_are_not_ones():
    """C = +inf at alpha 1.25: a check whose other entries are all infinite sends DBL_MAX x 1.25 = inf, and inf - inf is a NaN posterior.
    (At alpha <= 1 the clamp to DBL_MAX keeps every check-to-bit message finite and no NaN appears.)"""
    c = gu.edge_channel_case("hamming3", 1.25, freeze_llr=np.inf)
    got = gu.expected("edge_channel|hamming3|1.25|inf", c)
    assert got[3].any() and not got[3].all()
    nan = np.isnan(got[1])
    print(f"C = inf on hamming3: {int(nan.sum())} NaN posteriors in {int(nan.any(axis=1).sum())} rows")
    assert nan.any(), "the case shows no NaN"
    assert (got[0][nan] == 0).all(), "NaN <= 0 is false: the decision is 0"
    other = gu.expected("edge_channel|hamming3|1.25", gu.edge_channel_case("hamming3", 1.25))
    assert not bits_equal(got[1], other[1]), "C = inf and C = 25 give the same posteriors: the case shows nothing"


def test_scaling_factor_zero_round_0_is_the_plain_decodes_start():
    """The adaptive alpha (scaling factor 0): the rows solved in round 0 are the plain decode's, and later rounds solve more."""
    c = fu.bb144_case()
    got = gu.bpgd_restatement(c["h"], c["probs"], c["synd"][:16], 3, 4, 25.0, 0.0)
    plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"][:16], 3, 0.0, np.float64)
    first = got[2] <= 3
    assert first.any() and not first.all() and (got[3] & ~first).any()
    _equal(tuple(x[first] for x in got), tuple(x[first] for x in plain), "rows solved in round 0")


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------------
def test_decimation_schedule_and_decoder_arguments():
    from ldpc_amd import codes
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.bpgd_decoder import BpgdDecoder, decimation_schedule
    assert decimation_schedule(144) == (5, 144, 25.0)
    assert decimation_schedule(7, round_iters=3, max_rounds=16, freeze_llr=np.inf) == (3, 16, np.inf)
    assert decimation_schedule(7, max_rounds=1) == (5, 1, 25.0)
    for bad in (dict(round_iters=0), dict(round_iters=-1), dict(round_iters=2.5), dict(round_iters=True), dict(max_rounds=0), dict(max_rounds=1.5),
                dict(freeze_llr=0.0), dict(freeze_llr=-3.0), dict(freeze_llr=float("nan")), dict(freeze_llr=-np.inf), dict(freeze_llr="x"),
                dict(round_iters=2 ** 16, max_rounds=2 ** 15)):
        with pytest.raises(ValueError):
            decimation_schedule(7, **bad)
    assert decimation_schedule(7, round_iters=2 ** 15, max_rounds=2 ** 15) == (2 ** 15, 2 ** 15, 25.0), "2^30 fits"
    h = codes.hamming_code(3)
    d = BpgdDecoder(h, error_rate=0.1, round_iters=4, freeze_llr=30.0)
    assert (d.round_iters, d.max_rounds, d.freeze_llr) == (4, 7, 30.0) and d.bp_method == "minimum_sum" and d.schedule == "parallel"
    assert d.decimation == dict(round_iters=4, max_rounds=7, freeze_llr=30.0)
    assert d._engine is None, "construction needs no handle"
    with pytest.raises(ValueError):
        BpgdDecoder(h)
    with pytest.raises(ValueError):
        BpgdDecoder(h, error_rate=0.1, round_iters=0)
    with pytest.raises(ValueError, match="Unknown parameter"):
        BpgdDecoder(h, error_rate=0.1, max_iter=5)
    # the property of BpDecoder: round trip, None switches back, anything but a dict is an error
    b = BpDecoder(h, error_rate=0.1, bp_method="minimum_sum", max_iter=5)
    assert b.decimation is None
    with pytest.raises(ValueError, match="decimation is not set"):
        b.decimation_route
    b.decimation = dict(round_iters=3)
    assert b.decimation == dict(round_iters=3, max_rounds=7, freeze_llr=25.0)
    b.decimation = dict(round_iters=2, max_rounds=9, freeze_llr=np.inf)
    assert b.decimation == dict(round_iters=2, max_rounds=9, freeze_llr=np.inf)
    for bad in ([1, 2], 5, dict(rounds=3), dict(round_iters=0)):
        with pytest.raises((ValueError, TypeError)):
            b.decimation = bad
    assert b.decimation == dict(round_iters=2, max_rounds=9, freeze_llr=np.inf), "a refused value leaves what was set"
    b.decimation = None
    assert b.decimation is None and b._engine is None


def test_lane_edge_route_without_a_handle():
    from ldpc_amd import codes
    from ldpc_amd.bpgd_decoder import lane_edge_route
    from ldpc_amd.codes import synthetic
    assert lane_edge_route(codes.rep_code(5)) == "bp_edge"
    assert lane_edge_route(synthetic.rotated_surface_code_x(5)) == "bp_edge"
    assert lane_edge_route(codes.hamming_code(3)) == "bp_edge8"
    assert lane_edge_route(fu.bb144_case()["h"]) == "bp_edge8"
    assert lane_edge_route(fu.irregular_case()["h"]) == "unavailable"
    assert lane_edge_route(fu.heavy_rows_case()["h"]) == "unavailable"


def test_python_refusals_need_no_handle():
    """What guided decimation cannot do is a NotImplementedError at decode time, each with its reason, before any handle exists."""
    import scipy.sparse as sp
    from ldpc_amd import codes
    from ldpc_amd.bp_decoder import BpDecoder, SoftInfoBpDecoder
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    from ldpc_amd.bpgd_decoder import BpgdDecoder
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    h = codes.hamming_code(3)
    gd = dict(round_iters=3, max_rounds=4)
    synd = np.ones((2, 3), np.uint8)

    def decoder(**kw):
        d = BpDecoder(h, error_rate=0.1, **dict(dict(bp_method="minimum_sum", max_iter=5, input_vector_type="syndrome"), **kw))
        d.decimation = gd
        return d
    for kw, text in ((dict(bp_method="product_sum"), "product_sum"), (dict(schedule="serial"), "schedule='serial'"),
                     (dict(schedule="serial_relative"), "schedule='serial_relative'"), (dict(random_serial_schedule=True, schedule="serial"), "random_serial_schedule"),
                     (dict(device_ids=[0]), "device_ids")):
        d = decoder(**kw)
        with pytest.raises(NotImplementedError, match=f"decimation with .*{text}"):
            d.decode_batch(synd)
        assert d._engine is None
    d = decoder()
    d.message_dtype = "float32"
    with pytest.raises(NotImplementedError, match="decimation with message_dtype='float32'"):
        d.decode_batch(synd)
    d.message_dtype = "float64"
    with pytest.raises(NotImplementedError, match="decimation with channel_probs"):
        d.decode_batch(synd, channel_probs=np.full((2, 7), 0.1))
    d.memory_strength = 0.1
    with pytest.raises(NotImplementedError, match="decimation with memory_strength"):
        d.decode_batch(synd)
    d.memory_strength = None
    d.relay = dict(num_sets=2, pre_iter=4, set_max_iter=3)
    with pytest.raises(NotImplementedError, match="decimation with relay"):
        d.decode_batch(synd)
    assert d._engine is None
    # a code neither lane = edge family takes: refused with the follow-ups named, and the route says so
    big = fu.irregular_case()
    g = BpgdDecoder(big["h"], error_rate=0.03, round_iters=3, max_rounds=4, ms_scaling_factor=0.625)
    assert g.route == "unavailable"
    with pytest.raises(NotImplementedError, match="neither lane = edge kernel family takes this code.*lane = node route"):
        g.decode_batch(big["synd"][:2])
    assert g._engine is None
    s = SoftInfoBpDecoder(h, error_rate=0.1, max_iter=5, bp_method="minimum_sum", cutoff=2.0, sigma=1.0)
    s.decimation = gd
    with pytest.raises(NotImplementedError, match="decimation with soft-syndrome"):
        s.decode(np.ones(3))
    for method in ("osd_e", "osd_cs"):
        o = BpOsdDecoder(h, error_rate=0.1, max_iter=5, bp_method="minimum_sum", osd_method=method, osd_order=2)
        o.decimation = gd
        with pytest.raises(NotImplementedError, match="decimation with osd_method"):
            o.decode_batch(synd)
        assert o._engine is None
    model = (sp.csr_matrix(h), sp.csr_matrix(np.ones((1, 7), np.uint8)), np.full(7, 0.1))
    with pytest.raises(NotImplementedError, match="decimation with relay"):
        MonteCarloDemSimulation(model, target_run_count=10, decimation=gd, relay=dict(num_sets=2, pre_iter=4, set_max_iter=3))
    with pytest.raises(NotImplementedError, match="decimation with memory_strength"):
        MonteCarloDemSimulation(model, target_run_count=10, decimation=gd, memory_strength=0.1)
    with pytest.raises(NotImplementedError, match="decimation with osd_method OSD_E / OSD_CS"):
        MonteCarloDemSimulation(model, target_run_count=10, decimation=gd, osd_method="osd_cs", osd_order=2)
    with pytest.raises(ValueError, match="Invalid decimation"):
        MonteCarloDemSimulation(model, target_run_count=10, decimation=[3, 4])

    class Windows:  # (what MonteCarloDemSimulation asks of a window decoder before it refuses the combination)
        num_detectors = 3
        logical_observables_matrix = model[1]

        def predict_on_device(self, dets):
            raise AssertionError("never called")
    with pytest.raises(NotImplementedError, match="decimation with a window_decoder"):
        MonteCarloDemSimulation(model, target_run_count=10, decimation=gd, window_decoder=Windows())
    sim = MonteCarloDemSimulation(model, target_run_count=10, decimation=gd)
    assert sim.decimation == (3, 4, 25.0) and sim._engine is None


def test_symbols_and_the_ldpc_alias():
    from ldpc_amd import _lib
    for name in ("ldpc_hip_bp_set_decimation", "ldpc_hip_bp_get_decimation", "ldpc_hip_bp_decimation_route"):
        assert name in _lib.SYMBOLS
    import inspect
    import ldpc_amd
    from ldpc_amd.bpgd_decoder import BpgdDecoder
    assert BpgdDecoder.__mro__[1].__name__ == "BpDecoder"
    # as for ldpc_amd.relay_decoder: the reference has no such decoder, so install_as_ldpc names none; ldpc.bpgd_decoder resolves through the alias finder like any sub-package
    assert "bpgd" not in inspect.getsource(ldpc_amd.install_as_ldpc).lower()
    spec = ldpc_amd._LdpcAliasFinder().find_spec("ldpc.bpgd_decoder")
    assert spec is not None and spec.origin == "alias of ldpc_amd.bpgd_decoder"
