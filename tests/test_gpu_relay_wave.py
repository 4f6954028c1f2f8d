"""Relay-BP and memory min-sum on the lane = node kernel (bp_wave_relay_kernel; DESIGN.md sections 7c, 7d) against the NumPy restatements
(tests/relay_bp_util.py, tests/mem_bp_util.py), bit for bit and without a row left out: every instantiation once, the leg loop on the same
batch, the default mode and ldpc_hip_bp_relay_route, the work pools and the state a wavefront restarts with, the scaling factor 0, syndrome
bytes above 1, infinite and zero priors, the memory decode on the same kernel, on / off / on, and what goes round it (BP + OSD-0, the detector
error model loop).  The cases are tests/relay_wave_util.py's; every comparison first asserts on the restatement's output that it shows something."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import f32_util as fu
import launch_util
import mem_bp_util as mu
import relay_bp_util as ru
import relay_wave_util as wu
from oracle import bits_equal
from test_gpu_relay_bp import EDGE_MEM, EDGE_RELAY, LEG_LOOP, PLAIN_BP, _assert_edge_relay, _assert_leg_loop, _decode, _engine, _same

pytestmark = pytest.mark.gpu

PER_PASS_MEM = ("bp_spread_mem_init_kernel", "bp_spread_mem_bit_kernel", "bp_spread_mem_finish_kernel")
MODES = {4: False, 5: True}  # small-code kernel mode -> TEAM


def _name(rung, team):
    return f"bp_wave_relay_kernel<{rung[0]}, {rung[1]}, {'true' if team else 'false'}>"


def _assert_wave(log, name):
    launch_util.assert_resolved(log)
    got = launch_util.of(log, "bp_wave_relay_kernel")
    assert got == [name] and log[name] == 1, f"expected exactly {name}, once; the log has {sorted(log.items())}"
    launch_util.assert_ran(log, "wave_relay_table_kernel", "wave_prior_pad_kernel")
    launch_util.assert_not_ran(log, *LEG_LOOP, *EDGE_RELAY, *EDGE_MEM, *PLAIN_BP, "bp_spread_check_kernel", "bp_spread_synd_kernel")


# ---- 1. every instantiation once ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(wu.CASES))
def test_every_instantiation(name, mode):
    """B = 70, legs of (8, 4, 4, 4) iterations, stop after 2: decisions, posteriors, iteration counts and flags are the restatement's, from ONE
    launch of the rung's instantiation -- one wavefront per syndrome under mode 4, a team under mode 5.  (Fails without the kernel: the leg loop runs.)"""
    c, want = wu.batch70(name)
    ru.assert_shows_something(want, c["stop_after"], f"{name}/70")
    got, log = _decode(c, mode=mode)
    _same(got, want, f"{name} mode {mode}")
    _assert_wave(log, _name(wu.CASES[name][0], MODES[mode]))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["surface23", "hgp400"])
def test_a_later_lighter_solution_replaces_an_earlier_one(name, mode):
    """Six legs of (12, 6, 6, 6, 6, 6), stop after 3, all 300 rows: rows whose later solution replaced an earlier one, in both forms."""
    c, want = wu.case(name, 6), wu.want(name, 6)
    ru.assert_shows_something(want, c["stop_after"], f"{name}/300, six legs", need_replaced=True)
    got, log = _decode(c, mode=mode)
    _same(got, want, f"{name}, six legs, mode {mode}")
    _assert_wave(log, _name(wu.CASES[name][0], MODES[mode]))


# ---- 2. the same batch on the leg loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 6])
def test_modes_0_and_6_keep_the_leg_loop(mode):
    c, want = wu.batch70("ldpc200_36")
    got, log = _decode(c, mode=mode)
    _same(got, want, f"ldpc200_36 mode {mode}")
    _assert_leg_loop(log, len(c["leg_iters"]))


# ---- 3. the default mode -------------------------------------------------------------------------------------------------------------------------
def test_default_mode_takes_the_route_it_names():
    """Mode -1: relay_route() names the route the log then shows -- the lane = node kernel by the rule stated before the measurement (it beat the
    leg loop 48x on both measured codes) -- and a lane = edge code still launches its own relay kernel."""
    c, want = wu.batch70("hgp400")
    eng = _engine(c)
    try:
        route = eng.relay_route(70)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
    finally:
        eng.close()
    _same(got, want, "hgp400, default mode")
    # the measured default: the lane = node route; 70 rows are fewer than a wavefront slot each -- a team per syndrome
    assert route == "bp_wave_team"
    _assert_wave(log, _name((8, 4), True))
    # a lane = edge code is untouched
    full = ru.edge_case("bb144")
    e = ru.first_rows(full, 70)
    eng = _engine(e)
    try:
        assert eng.relay_route(70) == "bp_edge8"
        with launch_util.launch_log() as log:
            got = eng.decode_batch(e["synd"])
    finally:
        eng.close()
    _same(got, ru.rows_of(ru.expected("bb144", full), 70), "bb144, default mode")
    _assert_edge_relay(log, "bp_edge8_relay_kernel<9, 3>")


# ---- 4. the work pools, and what a wavefront starts its next syndrome with ---------------------------------------------------------------------
@pytest.mark.parametrize("rows,mode", [(1, 4), (1, 5), (4100, 5), (8200, 4)])
def test_batches_around_the_grid(rows, mode):
    """The (8,8) code: one row; 4 100 rows on teams (more than the 2 048 resident ones: the work counter); 8 200 rows on single wavefronts
    (more than 256 x 16 resident ones: the pools) -- the 300 rows tiled, so every wavefront decodes rows of every kind one after the other."""
    ru.assert_shows_something(wu.want("ldpc64_58"), 2, "ldpc64_58/300")
    c, want = wu.tiled("ldpc64_58", rows)
    got, log = _decode(c, mode=mode)
    _same(got, want, f"ldpc64_58, {rows} rows, mode {mode}")
    _assert_wave(log, _name((8, 8), MODES[mode]))


# ---- 5. scaling factor 0; syndrome bytes above 1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_scaling_factor_zero_counts_the_legs_iterations(mode):
    c, _ = wu.batch70("ldpc200_36")
    c = dict(c, alpha=0.0)
    want = ru.expected("wave|ldpc200_36|alpha0|70", c)
    assert want[3].any() and not want[3].all() and (want[2] > c["leg_iters"][0]).any()
    got, log = _decode(c, mode=mode)
    _same(got, want, f"alpha 0, mode {mode}")
    _assert_wave(log, _name((6, 3), MODES[mode]))


@pytest.mark.parametrize("mode", list(MODES))
def test_a_syndrome_byte_above_one_never_converges(mode):
    c, _ = wu.batch70("ldpc200_36")
    synd = c["synd"].copy()
    synd[3, 5], synd[9, 0], synd[64, 99] = 2, 3, 2
    c = dict(c, synd=synd)
    want = ru.expected("wave|ldpc200_36|bytes|70", c)
    for b in (3, 9, 64):
        assert not want[3][b] and want[2][b] == sum(c["leg_iters"])
    assert want[3].any()
    got, _ = _decode(c, mode=mode)
    _same(got, want, f"bytes > 1, mode {mode}")


# ---- 6. extreme priors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_extreme_priors(mode):
    """The (8,8) code with columns at p = 0, 1, 0.5 and 1e-300 (priors +inf, -inf, +0.0, 690.8), strength 0 on the infinite ones: the select
    returns a untouched where a + 0 * inf would be NaN."""
    base = wu.case("ldpc64_58")
    h = base["h"]
    probs = base["probs"].copy()
    probs[[0, 1, 2, 3, 17, 40, 41, 63]] = [0.0, 1.0, 0.5, 1e-300, 1.0, 0.0, 0.5, 1e-300]
    errors = (np.random.default_rng(5).random((70, h.shape[1])) < probs).astype(np.uint8)
    c = dict(base, probs=probs, synd=np.ascontiguousarray((errors @ h.T.toarray().astype(np.uint8)) & 1, np.uint8), gamma=ru.masked_strengths(probs, 4))
    assert (c["gamma"][:, [0, 1, 17, 40]] == 0.0).all() and (c["gamma"][1:, [2, 3]] != 0.0).all()
    want = ru.expected("wave|ldpc64_58|extreme", c)
    print(f"extreme priors: {ru.shows(want, 2)}")
    assert want[3].any() and not want[3].all() and (want[2] > c["leg_iters"][0]).any()
    assert not np.isnan(want[1][want[3]]).any()
    got, log = _decode(c, mode=mode)
    _same(got, want, f"extreme priors, mode {mode}")
    _assert_wave(log, _name((8, 8), MODES[mode]))


# ---- 7. the memory decode on the same kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["surface23", "hgp400"])
def test_memory(name, mode):
    base = wu.case(name)
    c = dict(h=base["h"], probs=base["probs"], synd=np.ascontiguousarray(base["synd"][:70]), max_iter=12, alpha=wu.ALPHA)
    g = mu.mixed_gamma(c["probs"])
    want = mu.expected(f"wave|{name}|mixed", c, g)
    plain = mu.plain(f"wave|{name}", c)
    mu.assert_shows_something(want, plain, c["max_iter"], f"{name}/mixed")
    kernel = _name(wu.CASES[name][0], MODES[mode])
    eng = _engine(c, relay=False, mode=mode)
    try:
        eng.set_memory(g)
        assert eng.relay_route(70) == ("bp_wave_team" if MODES[mode] else "bp_wave")
        with launch_util.launch_log() as log:
            mem = eng.decode_batch(c["synd"])
        _same(mem, want, f"{name} memory, mode {mode}")
        _assert_wave(log, kernel)
        launch_util.assert_not_ran(log, *PER_PASS_MEM)
        eng.set_memory(np.zeros(len(g)))
        with launch_util.launch_log() as log:
            zero = eng.decode_batch(c["synd"])
        _same(zero, plain, "all-zero strengths against the plain FP64 decode")
        _assert_wave(log, kernel)
        eng.set_memory(None)
        eng.set_relay(g[None, :], [c["max_iter"]], 1)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, tuple(np.asarray(x) if k != 3 else np.asarray(x, bool) for k, x in enumerate(mem)), "one relay leg against the memory decode")
        _assert_wave(log, kernel)
    finally:
        eng.close()


# ---- 8. on, off, on again; new channel probabilities; buffers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_on_off_on_again(mode):
    from ldpc_amd import _lib
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    c, want1 = wu.batch70("bb288")
    c2 = dict(c, gamma=ru.drawn_strengths(c["h"].shape[1], 3, seed=8), leg_iters=(9, 5, 5), stop_after=1)
    want2 = ru.expected("wave|bb288|second|70", c2)
    assert want2[3].any() and not want2[3].all() and not bits_equal(want1[1], want2[1])
    plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], 12, c["alpha"], np.float64)
    other = dict(c, probs=c["probs"][::-1].copy())
    want3 = ru.expected("wave|bb288|reversed|70", other)
    assert not bits_equal(want1[1], want3[1])
    kernel = _name((6, 3), MODES[mode])
    eng = _engine(c, relay=False, mode=mode)
    try:
        with launch_util.launch_log() as log0:
            got = eng.decode_batch(c["synd"])
        _same(got, plain, "before the relay")
        launch_util.assert_not_ran(log0, "bp_wave_relay_kernel", *LEG_LOOP)
        without = held()
        eng.set_relay(c["gamma"], c["leg_iters"], c["stop_after"])
        _same(eng.decode_batch(c["synd"]), want1, "first relay")
        assert held() > without
        eng.set_relay(None)
        assert held() == without, "set_relay(None) releases the padded tables"
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, plain, "relay off again")
        assert log == log0, f"with the relay off the handle launches {sorted(log.items())}, before it was ever set {sorted(log0.items())}"
        eng.set_relay(c2["gamma"], c2["leg_iters"], c2["stop_after"])
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, want2, "second relay")
        _assert_wave(log, kernel)
        eng.set_relay(c["gamma"], c["leg_iters"], c["stop_after"])
        eng.set_channel(other["probs"])
        _same(eng.decode_batch(c["synd"]), want3, "after set_channel")
    finally:
        eng.close()
    assert held() == before, f"{held() - before} bytes of device buffers outlive the handle"


# ---- 9. around it: BP + OSD-0, the detector error model loop -------------------------------------------------------------------------------------
def test_bposd_osd0_with_the_relay(oracle_built):
    """Rows with a solution: the restatement's.  Rows without: H x = s, and OSD-0 of the host oracle on the restatement's posteriors."""
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    c, want = wu.batch70("hgp400")
    dec, llr, it, cv = want[:4]
    orc = oracle_built.BpOracle(c["h"], error_channel=c["probs"], max_iter=8, bp_method="minimum_sum", ms_scaling_factor=c["alpha"])
    expect = dec.copy()
    for b in np.flatnonzero(~cv):
        expect[b] = orc.osdw(c["synd"][b], llr[b], 1, 0)[0]
    d = BpOsdDecoder(c["h"], error_channel=list(c["probs"]), max_iter=8, bp_method="minimum_sum", ms_scaling_factor=c["alpha"], osd_method="osd_0")
    d.relay = dict(strengths=c["gamma"], pre_iter=8, set_max_iter=4, stop_nconv=2)
    d._get_engine().set_small_code_kernel(5)
    assert d.relay_route == "bp_wave_team"
    with launch_util.launch_log() as log:
        got = d.decode_batch(c["synd"])
    _same((got, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), (expect, llr, it, cv), "BpOsdDecoder with the relay")
    _assert_wave(log, _name((8, 4), True))
    hd = c["h"].toarray().astype(np.int64)
    left = np.flatnonzero(~cv)
    assert len(left) and np.array_equal((got[left].astype(np.int64) @ hd.T) & 1, c["synd"][left]), "an OSD row does not satisfy H x = s"


def test_simulate_b8_and_the_monte_carlo_class_with_the_relay():
    """bb144 x 3 rounds, Relay-BP + OSD-0 on the one-wavefront form: both counters equal twin -> relay decode_b8 -> compare, for chunks 3000
    and 64; the decode_b8 flags and iteration counts are the restatement's."""
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from ldpc_amd.relay_decoder import relay_schedule
    from test_dem_sampler_twin import unpack
    from test_gpu_dem_sampler import SEED, engine, model, twin
    check, obs, pri = model("bb144x3")
    relay = dict(gamma0=0.125, pre_iter=8, num_sets=3, set_max_iter=4, stop_nconv=2, seed=11)
    g, li, stop = relay_schedule(check.shape[1], **relay)
    eng = engine(check, pri, obs)
    try:
        eng.set_small_code_kernel(4)
        eng.set_osd(1, 0)
        eng.set_relay(g, li, stop)
        _, dets, true_obs = twin("bb144x3", False, 0)
        with launch_util.launch_log() as log:
            pred, _, iters, conv = eng.decode_b8(np.array(dets), with_osd=True)
        assert launch_util.of(log, "bp_wave_relay_kernel") == [_name((8, 4), False)]
        launch_util.assert_not_ran(log, *LEG_LOOP, *PLAIN_BP, *EDGE_MEM, *EDGE_RELAY)
        synd = unpack(np.array(dets), check.shape[0])
        ref = ru.relay_restatement(check, np.clip(pri, 1e-9, 1 - 1e-9), g, li, stop, synd, 0.625)
        assert ref[3].any() and not ref[3].all() and (ref[2] > 8).any()
        ref_iters = np.where(synd.any(axis=1), ref[2], 0)  # (decode_b8: all-zero rows take the shortcut -- converged, 0 iterations)
        assert np.array_equal(np.asarray(conv, bool), ref[3] | ~synd.any(axis=1)) and np.array_equal(np.asarray(iters), ref_iters), \
            "decode_b8 with the relay: flags or iteration counts"
        want = (int(np.count_nonzero((pred != true_obs).any(axis=1))), int(np.count_nonzero(~np.asarray(conv, bool))))
        print(f"bb144x3 with the relay + OSD-0: {want[0]} logical failures, {want[1]} rows left without a solution, of 3000")
        assert want[1] > 0
        for chunk in (3000, 64):
            assert eng.simulate_b8(SEED, 0, 3000, chunk=chunk, with_osd=True) == want, f"chunk {chunk}"
    finally:
        eng.close()
    sim = MonteCarloDemSimulation((check, obs, pri), target_run_count=3000, batch_size=1024, seed=SEED, max_iter=12, relay=relay)
    sim._get_engine().set_small_code_kernel(4)
    got = sim.run()
    assert (got["fail_count"], got["bp_unconverged_count"]) == want


# ---- 10. ldpc_hip_bp_relay_route ---------------------------------------------------------------------------------------------------------------
def test_relay_route():
    from ldpc_amd import _lib
    from ldpc_amd.relay_decoder import RelayBpDecoder
    c = wu.case("ldpc64_58")
    eng = _engine(c, relay=False)
    lib = eng._lib
    route = C.c_int32(-7)
    try:
        # neither mode on: LDPC_HIP_ERR_INVALID, the word untouched
        assert lib.ldpc_hip_bp_relay_route(eng._h, 70, C.byref(route)) == -1 and route.value == -7 and b"neither" in lib.ldpc_hip_last_error()
        with pytest.raises(ValueError, match="neither"):
            eng.relay_route(70)
        assert lib.ldpc_hip_bp_relay_route(None, 70, C.byref(route)) == -1 and lib.ldpc_hip_bp_relay_route(eng._h, 70, None) == -1
        eng.set_relay(c["gamma"], c["leg_iters"], c["stop_after"])
        assert lib.ldpc_hip_bp_relay_route(eng._h, -1, C.byref(route)) == -1
        with launch_util.launch_log() as log:
            for mode, want in ((0, "per_pass"), (6, "per_pass"), (2, "per_pass"), (4, "bp_wave"), (5, "bp_wave_team"), (-1, "bp_wave_team"), (1, "bp_wave_team")):
                eng.set_small_code_kernel(mode)
                assert eng.relay_route(70) == want, f"mode {mode}"
            eng.set_small_code_kernel(3)  # the plan's own choice: a team for a batch of one syndrome per wavefront slot at most, else single wavefronts
            assert eng.relay_route(1) == "bp_wave_team" and eng.relay_route(1 << 20) == "bp_wave"
            # the memory answers through the same function
            eng.set_relay(None)
            eng.set_memory(mu.mixed_gamma(c["probs"]))
            eng.set_small_code_kernel(4)
            assert eng.relay_route(70) == "bp_wave"
            eng.set_memory(None)
            # a refused decode launches nothing
            eng.set_relay(c["gamma"], c["leg_iters"], c["stop_after"])
            eng.set_params(12, 0, 1.0)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: Relay-BP: product-sum"):
                eng.decode_batch(c["synd"][:70])
        assert not log, f"asking for the route, or a refused decode, launched something: {sorted(log)}"
    finally:
        eng.close()
    for code, want in (("surface5", "bp_edge"), ("bb144", "bp_edge8")):
        e = ru.first_rows(ru.edge_case(code), 70)
        eng = _engine(e)
        try:
            assert eng.relay_route(70) == want
            eng.set_small_code_kernel(5)
            assert eng.relay_route(70) == want, "the lane = edge families come first in every mode but 0"
            eng.set_small_code_kernel(0)
            assert eng.relay_route(70) == "per_pass"
        finally:
            eng.close()
    irr = fu.irregular_case()  # columns of 11: no on-chip kernel
    eng = _engine(dict(irr, gamma=ru.masked_strengths(irr["probs"], 2), leg_iters=(4, 4), stop_after=1), mode=5)
    try:
        assert eng.relay_route(130) == "per_pass"
    finally:
        eng.close()
    # the decoder classes: the batch size last decoded, or 1
    b, want = wu.batch70("ldpc64_58")
    some = np.flatnonzero(b["synd"].any(axis=1))  # (an all-zero row takes the decoder's host shortcut: converged, 0 iterations)
    b, want, rows = dict(b, synd=np.ascontiguousarray(b["synd"][some])), ru.take(want, some), len(some)
    assert rows >= 64 and want[3].any() and not want[3].all()
    d = RelayBpDecoder(b["h"], channel_probs=b["probs"], ms_scaling_factor=b["alpha"], strengths=b["gamma"], pre_iter=8, set_max_iter=4, stop_nconv=2)
    d._get_engine().set_small_code_kernel(3)
    assert d.route == "bp_wave_team" and d.relay_route == d.route
    dec = d.decode_batch(np.tile(b["synd"], (130, 1)))
    assert d.route == "bp_wave"
    _same((dec[:rows], d.log_prob_ratios_batch[:rows], d.iter_batch[:rows], d.converge_batch[:rows]), want, "RelayBpDecoder on the lane = node kernel")
    d.relay = None
    with pytest.raises(ValueError, match="neither"):
        d.relay_route
