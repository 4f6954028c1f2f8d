"""Relay-BP without a GPU: the NumPy restatement (tests/relay_bp_util.py) against the memory and the plain restatements where it must equal
them, the weight tree against math.fsum and against a second implementation, the bookkeeping of the legs on the repetition code, that the
shared cases show what the GPU tests need, and the argument errors of the Python layer -- each before any handle exists."""
import math

import numpy as np
import pytest

import f32_util as fu
import mem_bp_util as mu
import relay_bp_util as ru
from oracle import bits_equal


def _equal(got, want, what):
    for k, name in ((0, "decoding"), (2, "iterations"), (3, "converge")):
        assert np.array_equal(got[k], want[k]), f"{what}: {name}"
    assert bits_equal(got[1], want[1]), f"{what}: log-ratios differ in some bit"


# ---- the two invariants ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["hamming3", "rep5", "irregular", "bb144"])
def test_one_leg_is_the_memory_decode(key):
    """One leg of max_iter iterations, stop after 1: mem_bp_util.min_sum_memory_restatement, bit for bit."""
    c = {"hamming3": lambda: fu.small_case("hamming3", 0.625), "rep5": lambda: fu.small_case("rep5", 0.0), "irregular": fu.irregular_case,
         "bb144": lambda: mu.first_rows(mu.edge_case("bb144"), 70)}[key]()
    g = mu.mixed_gamma(c["probs"])
    want = mu.min_sum_memory_restatement(c["h"], c["probs"], g, c["synd"], c["max_iter"], c["alpha"])
    got = ru.relay_restatement(c["h"], c["probs"], g[None, :], [c["max_iter"]], 1, c["synd"], c["alpha"])
    _equal(got, want, key)
    assert want[3].any() and not want[3].all()


@pytest.mark.parametrize("key", ["hamming3", "rep5", "irregular"])
def test_all_strengths_zero_one_leg_is_the_plain_decode(key):
    c = {"hamming3": lambda: fu.small_case("hamming3", 0.625), "rep5": lambda: fu.small_case("rep5", 0.0), "irregular": fu.irregular_case}[key]()
    want = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], c["max_iter"], c["alpha"], np.float64)
    got = ru.relay_restatement(c["h"], c["probs"], np.zeros((1, c["h"].shape[1])), [c["max_iter"]], 1, c["synd"], c["alpha"])
    _equal(got, want, key)
    assert want[3].any() and not want[3].all()


# ---- the weight ----------------------------------------------------------------------------------------------------------------------------------
def _weight_again(dec, l0):
    """The same tree, written lane by lane with Python floats (IEEE doubles, one rounding per addition)."""
    n = len(dec)
    p = []
    for lane in range(64):
        acc = 0.0
        for j in range(lane, n, 64):
            acc = acc + (float(l0[j]) if dec[j] else 0.0)
        p.append(acc)
    for s in (1, 2, 4, 8, 16, 32):
        p = [p[lane] + p[lane ^ s] for lane in range(64)]
    return p[0]


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 144, 600, 1000])
def test_weight_tree(n):
    rng = np.random.default_rng(n)
    l0 = np.log((1 - (p := rng.uniform(0.001, 0.7, n))) / p)  # (some negative: p > 0.5)
    assert (l0 < 0).any() or n < 5
    decs = (rng.random((20, n)) < 0.3).astype(np.uint8)
    decs[0] = 0
    decs[1] = 1
    w = ru.relay_weight(decs, l0)
    for b in range(len(decs)):
        again = _weight_again(decs[b], l0)
        assert np.float64(again).view(np.uint64) == np.float64(w[b]).view(np.uint64), f"n = {n}, row {b}: the two trees differ"
        assert np.float64(ru.relay_weight(decs[b], l0)).view(np.uint64) == np.float64(w[b]).view(np.uint64), "one row against the batch"
        terms = [float(l0[j]) for j in range(n) if decs[b][j]]
        exact = math.fsum(terms)
        ulp = np.spacing(max([abs(t) for t in terms] + [abs(exact), 1e-300]) * max(len(terms), 1))
        assert abs(w[b] - exact) <= n * ulp, f"n = {n}, row {b}: {w[b]!r} against fsum {exact!r}"
    assert w[0] == 0.0 and not np.signbit(w[0])


def test_weight_is_a_select_not_a_product():
    """An undecided bit with an infinite prior contributes +0.0, not 0 * inf = NaN; a decided one contributes its infinity."""
    l0 = np.array([np.inf, -np.inf, 1.5, 0.0])
    assert ru.relay_weight(np.array([0, 0, 1, 1], np.uint8), l0) == 1.5
    assert ru.relay_weight(np.array([1, 0, 1, 0], np.uint8), l0) == np.inf
    assert np.isnan(ru.relay_weight(np.array([1, 1, 0, 0], np.uint8), l0))


# ---- the bookkeeping of the legs, on the repetition code -----------------------------------------------------------------------------------------
def _rep5_batch():
    """All 16 syndromes of the length-5 repetition code under four channels: every syndrome has exactly two solutions, x and its complement."""
    from ldpc_amd import codes
    h = codes.rep_code(5)
    synd = np.array([[(s >> i) & 1 for i in range(4)] for s in range(16)], np.uint8)
    return h, synd


def _by_hand(h, probs, gamma, leg_iters, stop_after, synd_row, alpha):
    """The loop of the module's docstring for ONE row, leg by leg, with the second weight implementation."""
    graph = ru._Graph(h)
    prior = fu.priors_f64(probs)
    m_prev, best, best_w, nsol, total, legs, last = None, None, math.inf, 0, 0, [], None
    for g, iters in zip(gamma, leg_iters):
        d, llr, it, cv = ru.memory_leg(graph, prior, mu.memory_a(probs, g), g, synd_row[None, :], m_prev, iters, alpha)
        total += int(it[0])
        m_prev = llr
        last = (d[0], llr[0])
        w = _weight_again(d[0], prior) if cv[0] else None
        legs.append((bool(cv[0]), w, d[0].copy()))
        if cv[0]:
            nsol += 1
            if w < best_w:
                best, best_w = last, w
            if nsol == stop_after:
                break
    return (best if nsol else last), total, nsol > 0, legs


def _rep5_runs():
    h, synd = _rep5_batch()
    rng = np.random.default_rng(3)
    for trial in range(12):
        probs = rng.uniform(0.3, 0.49, 5)  # (close to 1/2: the two solutions weigh nearly the same, and BP does not always find the lighter first)
        gamma = rng.uniform(-0.95, 0.9, (5, 5))
        if trial % 2 == 0:
            gamma[0] = 0.125
        for stop in (1, 2, 5):
            yield h, synd, probs, gamma, (3, 2, 2, 2, 2), stop


def test_rep5_bookkeeping():
    """Against the by-hand loop, row by row; and the four behaviours, each seen at least once: stop_after = 1 stops at the first solution; a later,
    strictly lighter solution replaces an earlier one; a later solution of equal (or larger) weight does not; no solution gives the last
    leg's outputs and converge = False."""
    seen = dict(stops_at_first=0, replaced=0, kept_first_of_equal=0, kept_lighter_first=0, no_solution=0)
    for h, synd, probs, gamma, leg_iters, stop in _rep5_runs():
        got = ru.relay_restatement(h, probs, gamma, leg_iters, stop, synd, 0.625, details=True)
        for b in range(len(synd)):
            (dec, llr), total, conv, legs = _by_hand(h, probs, gamma, leg_iters, stop, synd[b], 0.625)
            assert np.array_equal(got[0][b], dec) and bits_equal(got[1][b], llr) and got[2][b] == total and got[3][b] == conv, f"row {b}, stop {stop}"
            sols = [(k, w, d) for k, (cv, w, d) in enumerate(legs) if cv]
            if not sols:
                assert not conv and total == sum(leg_iters) and len(legs) == 5 and np.array_equal(dec, legs[-1][2])
                seen["no_solution"] += 1
                continue
            assert np.array_equal((dec.astype(int) @ h.toarray().T.astype(int)) & 1, synd[b]), "the chosen solution reproduces the syndrome"
            if stop == 1:
                assert len(legs) == sols[0][0] + 1 and len(sols) == 1 and np.array_equal(dec, sols[0][2])
                seen["stops_at_first"] += sols[0][0] + 1 < 5
            weights = [w for _, w, _ in sols]
            first_min = weights.index(min(weights))
            assert np.array_equal(dec, sols[first_min][2]), "the FIRST of the lightest solutions is the result"
            if first_min > 0:
                assert weights[first_min] < weights[0]
                seen["replaced"] += 1
            if len(sols) > 1 and first_min == 0:
                seen["kept_first_of_equal"] += any(w == weights[0] for w in weights[1:])
                seen["kept_lighter_first"] += any(w > weights[0] for w in weights[1:])
    print(seen)
    assert all(seen.values()), f"a behaviour was never seen: {seen}"


# ---- the shared cases show what the GPU tests need --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", ["surface5", "bb144", "hgp_hamming3"])
def test_edge_cases_show_something(code):
    full = ru.edge_case(code)
    want = ru.expected(code, full)
    ru.assert_shows_something(want, full["stop_after"], f"{code}/300", need_replaced=True)
    idx = ru.ragged_rows(want, full["stop_after"], 70)
    assert len(idx) == 70 and len(set(idx.tolist())) == 70
    ru.assert_shows_something(ru.take(want, idx), full["stop_after"], f"{code}/70", need_replaced=True)


def test_hgp_hamming3_counts_of_the_first_70_rows():
    """The figures the definition was first run with (uniform p, strengths seeded 7): 5 rows without a solution, 50 stopped at 3, 7 first
    solved after leg 0, 5 replaced."""
    want = ru.rows_of(ru.expected("hgp_hamming3", ru.edge_case("hgp_hamming3")), 70)
    none, stopped, _, late, replaced = ru.shows(want, 3)
    assert (none, stopped, late, replaced) == (5, 50, 7, 5)


# ---- the Python layer's argument errors ------------------------------------------------------------------------------------------------------------
def test_relay_schedule_and_decoder_arguments():
    from ldpc_amd import codes
    from ldpc_amd.relay_decoder import RelayBpDecoder, relay_schedule
    g, li, stop = relay_schedule(7)
    assert g.shape == (61, 7) and (g[0] == 0.125).all() and li.tolist() == [80] + [60] * 60 and stop == 1
    assert np.array_equal(g[1:], np.random.default_rng(0).uniform(-0.24, 0.66, (60, 7)))
    g, li, stop = relay_schedule(7, strengths=np.zeros((3, 7)), pre_iter=9, set_max_iter=4, stop_nconv=2)
    assert g.shape == (3, 7) and li.tolist() == [9, 4, 4] and stop == 2
    g, li, _ = relay_schedule(7, num_sets=0, pre_iter=5)
    assert g.shape == (1, 7) and li.tolist() == [5]
    for bad in (dict(pre_iter=0), dict(set_max_iter=0), dict(stop_nconv=0), dict(num_sets=-1), dict(gamma0=1.0), dict(gamma0=float("nan")),
                dict(gamma_dist_interval=(-0.2, 1.0)), dict(gamma_dist_interval=(0.5, 0.1)), dict(strengths=np.zeros((2, 6))), dict(strengths=np.full((2, 7), -1.5)),
                dict(pre_iter=2.5), dict(seed=-1)):
        with pytest.raises(ValueError):
            relay_schedule(7, **bad)
    h = codes.hamming_code(3)
    d = RelayBpDecoder(h, error_rate=0.1, num_sets=2, pre_iter=5, set_max_iter=4, stop_nconv=2, seed=4)
    assert d.strengths.shape == (3, 7) and d.leg_iters.tolist() == [5, 4, 4] and d.stop_nconv == 2 and d.bp_method == "minimum_sum" and d.schedule == "parallel"
    assert np.array_equal(d.strengths[1:], np.random.default_rng(4).uniform(-0.24, 0.66, (2, 7)))
    assert d._engine is None, "construction needs no handle"
    with pytest.raises(ValueError):
        RelayBpDecoder(h)
    with pytest.raises(ValueError):
        RelayBpDecoder(h, error_rate=0.1, stop_nconv=0)
    with pytest.raises(ValueError, match="Unknown parameter"):
        RelayBpDecoder(h, error_rate=0.1, max_iter=5)
    d.relay = None
    with pytest.raises(ValueError):
        d.relay = [1, 2]


def test_python_refusals_need_no_handle():
    """What Relay-BP cannot do is a NotImplementedError at decode time, each with its reason, before any handle exists."""
    import scipy.sparse as sp
    from ldpc_amd.bp_decoder import BpDecoder, SoftInfoBpDecoder
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from ldpc_amd import codes
    h = codes.hamming_code(3)
    relay = dict(num_sets=2, pre_iter=4, set_max_iter=3)
    synd = np.ones((2, 3), np.uint8)

    def decoder(**kw):
        d = BpDecoder(h, error_rate=0.1, **dict(dict(bp_method="minimum_sum", max_iter=5, input_vector_type="syndrome"), **kw))
        d.relay = relay
        return d
    for kw, text in ((dict(bp_method="product_sum"), "product_sum"), (dict(schedule="serial"), "schedule='serial'"), (dict(device_ids=[0]), "device_ids")):
        d = decoder(**kw)
        with pytest.raises(NotImplementedError, match=f"relay with .*{text}"):
            d.decode_batch(synd)
        assert d._engine is None
    d = decoder()
    d.message_dtype = "float32"
    with pytest.raises(NotImplementedError, match="relay with message_dtype='float32'"):
        d.decode_batch(synd)
    d.message_dtype = "float64"
    with pytest.raises(NotImplementedError, match="relay with channel_probs"):
        d.decode_batch(synd, channel_probs=np.full((2, 7), 0.1))
    d.memory_strength = 0.1
    with pytest.raises(NotImplementedError, match="relay with memory_strength"):
        d.decode_batch(synd)
    assert d._engine is None
    s = SoftInfoBpDecoder(h, error_rate=0.1, max_iter=5, bp_method="minimum_sum", cutoff=2.0, sigma=1.0)
    s.relay = relay
    with pytest.raises(NotImplementedError, match="relay with soft-syndrome"):
        s.decode(np.ones(3))
    model = (sp.csr_matrix(h), sp.csr_matrix(np.ones((1, 7), np.uint8)), np.full(7, 0.1))
    with pytest.raises(NotImplementedError, match="relay with memory_strength"):
        MonteCarloDemSimulation(model, target_run_count=10, relay=relay, memory_strength=0.1)
    with pytest.raises(NotImplementedError, match="OSD_E / OSD_CS"):
        MonteCarloDemSimulation(model, target_run_count=10, relay=relay, osd_method="osd_cs", osd_order=2)

    class Windows:  # (what MonteCarloDemSimulation asks of a window decoder before it refuses the combination)
        num_detectors = 3
        logical_observables_matrix = model[1]

        def predict_on_device(self, dets):
            raise AssertionError("never called")
    with pytest.raises(NotImplementedError, match="relay with a window_decoder"):
        MonteCarloDemSimulation(model, target_run_count=10, relay=relay, window_decoder=Windows())
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    for method in ("osd_e", "osd_cs"):
        o = BpOsdDecoder(h, error_rate=0.1, max_iter=5, bp_method="minimum_sum", osd_method=method, osd_order=2)
        o.relay = relay
        with pytest.raises(NotImplementedError, match="relay with osd_method"):
            o.decode_batch(synd)
        assert o._engine is None


def test_symbols_and_install_as_ldpc():
    from ldpc_amd import _lib
    assert "ldpc_hip_bp_set_relay" in _lib.SYMBOLS and "ldpc_hip_bp_get_relay" in _lib.SYMBOLS
    import ldpc_amd
    import inspect
    assert "relay" not in inspect.getsource(ldpc_amd.install_as_ldpc).lower(), "the reference has no relay decoder: nothing is installed under ldpc.*"
