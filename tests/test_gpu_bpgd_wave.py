"""BP with guided decimation on the lane = node kernel (bp_wave_gd_kernel; ldpc_hip_bp_set_decimation_lane_node) against
the NumPy restatement (tests/bpgd_util.py), bit for bit: hard decisions, the bit patterns of the posteriors, total iteration counts and converge
flags -- every instantiation once with the launch log showing which one ran, the default plan and the work pool into poisoned outputs, ties,
nothing left to freeze, special priors, an empty column, the invariants, the routing and the switch, and what goes round the engine.  The cases
are tests/bpgd_wave_util.py's; tests/test_bpgd_wave_cases.py asserts on the CPU that each shows what it is there for."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import bpgd_util as gu
import bpgd_wave_util as gw
import f32_util as fu
import ladder_util as lu
import launch_util
import relay_wave_util as wu
from test_gpu_bpgd import EDGE_GD, PLAIN_BP, _poisoned, _same

pytestmark = pytest.mark.gpu

MODES = {4: False, 5: True}  # small-code kernel mode -> TEAM
OLD_SENTENCE = r"neither lane = edge kernel family takes this code.*the lane = node route for larger codes and a per-pass route are not built yet"
NEW_SENTENCE = r"neither lane = edge kernel family nor the lane = node kernel takes this code.*a per-pass route is not built"


def _name(rung, team):
    return f"bp_wave_gd_kernel<{rung[0]}, {rung[1]}, {'true' if team else 'false'}>"


def _engine(c, gd=True, mode=None, lane_node=True, max_iter=12):
    from ldpc_amd.engine import HipBpEngine
    h = sp.csr_matrix(c["h"])
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], c["probs"], max_iter, 1, c["alpha"])
    if mode is not None:
        eng.set_small_code_kernel(mode)
    if lane_node:
        eng.set_decimation_lane_node(True)
    if gd:
        eng.set_decimation(c["round_iters"], c["max_rounds"], c["freeze_llr"])
    return eng


def _decode(c, mode=None):
    eng = _engine(c, mode=mode)
    try:
        with launch_util.launch_log() as log:
            out = eng.decode_batch(c["synd"])
    finally:
        eng.close()
    return out, log


def _assert_wave_gd(log, name):
    launch_util.assert_resolved(log)
    got = launch_util.of(log, "bp_wave_gd_kernel")
    assert got == [name] and log[name] == 1, f"expected exactly {name}, once; the log has {sorted(log.items())}"
    launch_util.assert_ran(log, "wave_prior_pad_kernel")
    launch_util.assert_not_ran(log, *PLAIN_BP, *EDGE_GD, "bp_spread_check_kernel", "bp_spread_synd_kernel")


def _both_modes(c, want, rung, what):
    for mode, team in MODES.items():
        got, log = _decode(c, mode=mode)
        _same(got, want, f"{what}, mode {mode}")
        _assert_wave_gd(log, _name(rung, team))


# ---- 1. every instantiation once ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(wu.CASES))
def test_every_instantiation(name, mode):
    """B = 70, T = 3, R = 6, C = 25: ONE launch of the rung's instantiation -- one wavefront per syndrome under mode 4, a team under mode 5."""
    c, want = gw.every_instantiation(name), gw.want_instantiation(name)
    assert gu.shows(want, gw.R) == gw.SHOWS[name]
    got, log = _decode(c, mode=mode)
    _same(got, want, f"{name} mode {mode}")
    _assert_wave_gd(log, _name(wu.CASES[name][0], MODES[mode]))


# ---- 2. the default plan and the work pool ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,want_llr", [(-1, True), (-1, False), (4, True), (4, False)])
def test_work_pool_into_poisoned_outputs(mode, want_llr):
    """20 011 rows, row b = the case's row b % 300: a row pulled from the pool starts from L0 and clear masks, not from its predecessor's."""
    import torch
    c, want = gw.tiled("ldpc64_58", gw.POOL_ROWS)
    synd = torch.as_tensor(c["synd"], device="cuda")
    eng = _engine(c, mode=mode)
    try:
        route = eng.decimation_route(gw.POOL_ROWS)
        out = _poisoned(gw.POOL_ROWS, c["h"].shape[1], want_llr)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(synd, want_llr=want_llr, out=out)
            torch.cuda.synchronize()
    finally:
        eng.close()
    assert all(g is o for g, o in zip(got, out))
    dec, llr, it, cv = (None if x is None else x.cpu().numpy() for x in got)
    if not want_llr:
        assert llr is None
        llr = want[1]
    assert set(np.unique(cv).tolist()) <= {0, 1}, "converge flags that were never written"
    _same((dec, llr, it, cv), want, f"ldpc64_58 x {gw.POOL_ROWS} rows, mode {mode}")
    assert route in ("bp_wave", "bp_wave_team") and (mode != 4 or route == "bp_wave")
    _assert_wave_gd(log, _name((8, 8), route == "bp_wave_team"))


@pytest.mark.parametrize("rows", [70, 300])
def test_default_mode_on_hgp400(rows):
    full, w = gw.all_rows("hgp400"), gw.want_all_rows("hgp400")
    c, want = dict(full, synd=np.ascontiguousarray(full["synd"][:rows])), gw.take(w, np.arange(rows))
    eng = _engine(c)
    try:
        route = eng.decimation_route(rows)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
    finally:
        eng.close()
    _same(got, want, f"hgp400, {rows} rows, default mode")
    assert route in ("bp_wave", "bp_wave_team")
    _assert_wave_gd(log, _name((8, 4), route == "bp_wave_team"))


# ---- 3. ties; 4. nothing left to freeze --------------------------------------------------------------------------------------------------------
def test_ties():
    c = gw.tie_case()
    want = gu.expected("wave_gd|tie", c)
    assert want[4]["frozen"].tolist() == [[2, 0, 1, 3, 4]] * 3
    _both_modes(c, want, (4, 2), "rep_code(258), ties")


def test_nothing_left_to_freeze():
    c = gw.all_frozen_case()
    want = gu.expected("wave_gd|all_frozen", c)
    assert (want[2] == 67).all() and (want[4]["frozen"][:, 64:] == -1).all()
    _both_modes(c, want, (8, 8), "ldpc64_58, R = n + 3")


# ---- 5. special priors; 6. an empty column -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,freeze", gw.SPECIAL)
def test_special_priors(alpha, freeze):
    c = gw.special_priors_case(alpha, freeze)
    want = gu.expected(f"wave_gd|special|{alpha}|{freeze}", c)
    assert want[3].any() and (want[4]["frozen"] >= 0).any()
    _both_modes(c, want, (8, 8), f"special priors, alpha {alpha}, C = {freeze}")


def test_an_empty_column():
    c = gw.empty_column_case()
    want = gu.expected("wave_gd|empty_column", c)
    assert (want[4]["frozen"] >= 0).any()
    _both_modes(c, want, (4, 2), "outside-empty-column")


# ---- 7. invariants --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_one_round_is_the_plain_decode(mode):
    c = gw.one_round_case()
    want = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], c["round_iters"], c["alpha"], np.float64)
    assert want[3].any() and not want[3].all()
    eng = _engine(c, gd=False, mode=mode, max_iter=c["round_iters"])
    try:
        plain = eng.decode_batch(c["synd"])
        eng.set_decimation(c["round_iters"], 1, 25.0)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
    finally:
        eng.close()
    _same(plain, want, "the plain decode against the plain restatement")
    _same(got, want, "R = 1 against the plain restatement")
    _assert_wave_gd(log, _name((6, 3), MODES[mode]))
    hd = c["h"].toarray().astype(np.int64)
    ok = np.flatnonzero(np.asarray(got[3], bool))
    assert len(ok) and np.array_equal((np.asarray(got[0])[ok].astype(np.int64) @ hd.T) & 1, c["synd"][ok]), "a converged row reproduces its syndrome"


@pytest.mark.parametrize("mode", list(MODES))
def test_converged_rows_reproduce_their_syndromes_and_off_launches_what_it_did_before(mode):
    from ldpc_amd import _lib
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    c, want = gw.every_instantiation("bb288"), gw.want_instantiation("bb288")
    plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], 12, c["alpha"], np.float64)
    eng = _engine(c, gd=False, mode=mode, lane_node=False)
    try:
        with launch_util.launch_log() as log0:
            got = eng.decode_batch(c["synd"])
        _same(got, plain, "before the switch was touched")
        launch_util.assert_not_ran(log0, "bp_wave_gd_kernel")
        without = held()
        eng.set_decimation_lane_node(True)
        eng.set_decimation(gw.T, gw.R, gw.C)
        got = eng.decode_batch(c["synd"])
        _same(got, want, "with the decimation")
        hd = c["h"].toarray().astype(np.int64)
        ok = np.flatnonzero(np.asarray(got[3], bool))
        assert len(ok) and np.array_equal((np.asarray(got[0])[ok].astype(np.int64) @ hd.T) & 1, c["synd"][ok]), "a converged row reproduces its syndrome"
        assert held() > without, "the padded priors are a buffer of the handle"
        eng.set_decimation(None)
        assert held() == without, "set_decimation(None) releases the padded priors"
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, plain, "decimation off again")
        assert log == log0, f"with the decimation off the handle launches {sorted(log.items())}, before the switch was touched {sorted(log0.items())}"
    finally:
        eng.close()


# ---- 8. routing and the switch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(wu.CASES))
def test_switch_off_is_todays_refusal(name):
    from ldpc_amd import _lib
    c = gw.every_instantiation(name)
    eng = _engine(c, lane_node=False)
    try:
        assert eng.decimation_lane_node is False
        with launch_util.launch_log() as log:
            assert eng.decimation_route(70) == "unavailable"
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: neither lane = edge kernel family takes this code under small-code kernel mode -1 "
                               r".*the lane = node route for larger codes and a per-pass route are not built yet"):
                eng.decode_batch(c["synd"])
        assert not log, f"a refused decode launched something: {sorted(log)}"
    finally:
        eng.close()


def test_routes_with_the_switch_on():
    from ldpc_amd import _lib
    from ldpc_amd.bpgd_decoder import lane_edge_route, lane_node_takes
    with launch_util.launch_log() as log:
        for name in wu.CASES:
            c = gw.every_instantiation(name)
            eng = _engine(c)
            try:
                assert eng.decimation_lane_node is True and lane_node_takes(c["h"])
                assert eng.decimation_route(70) in ("bp_wave", "bp_wave_team"), name
                for mode, want in ((4, "bp_wave"), (5, "bp_wave_team"), (0, "unavailable"), (6, "unavailable"), (2, "unavailable"), (1, eng.decimation_route(70))):
                    eng.set_small_code_kernel(mode)
                    assert eng.decimation_route(70) == want, f"{name} mode {mode}"
                eng.set_small_code_kernel(3)  # the plan's own choice: by the batch
                assert eng.decimation_route(1) == "bp_wave_team"
                eng.set_small_code_kernel(6)
                with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: neither lane = edge kernel family nor the lane = node kernel takes this code "
                                   r"under small-code kernel mode 6 .*a per-pass route is not built"):
                    eng.decode_batch(c["synd"])
                eng.set_decimation_lane_node(False)  # the setter forgets the route it knew
                eng.set_small_code_kernel(-1)
                assert eng.decimation_route(70) == "unavailable"
            finally:
                eng.close()
        # a lane = edge code keeps its family, in every mode but 0
        e = fu.bb144_case()
        eng = _engine(dict(e, round_iters=3, max_rounds=6, freeze_llr=25.0))
        try:
            for mode, want in ((-1, "bp_edge8"), (5, "bp_edge8"), (6, "bp_edge8"), (0, "unavailable")):
                eng.set_small_code_kernel(mode)
                assert eng.decimation_route(70) == want, f"bb144 mode {mode}"
        finally:
            eng.close()
        # rows of 20, columns of 11: no kernel, the new sentence
        for big in (fu.irregular_case(), fu.heavy_rows_case()):
            assert lane_edge_route(big["h"]) == "unavailable" and not lane_node_takes(big["h"])
            eng = _engine(dict(big, round_iters=3, max_rounds=4, freeze_llr=25.0))
            try:
                assert eng.decimation_route(70) == "unavailable"
                for kw in ({}, dict(osd0=True)):
                    with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: " + NEW_SENTENCE):
                        eng.decode_batch(big["synd"], **kw)
            finally:
                eng.close()
        # lane_node_takes is the library's answer
        for case in lu.OUTSIDE_CASES:
            h, probs, _ = lu.inputs(case.id)
            eng = _engine(dict(h=h, probs=np.array(probs), alpha=0.625, round_iters=2, max_rounds=2, freeze_llr=25.0))
            try:
                route = eng.decimation_route(70)
                assert (route != "unavailable") == (lane_edge_route(h) != "unavailable" or lane_node_takes(h)), case.id
                assert (route in ("bp_wave", "bp_wave_team")) == (lane_edge_route(h) == "unavailable" and lane_node_takes(h)), case.id
            finally:
                eng.close()
    assert not log, f"asking for the route, or a refused decode, launched something: {sorted(log)}"


def test_cabi_getter_and_setter():
    c = gw.every_instantiation("ldpc64_58")
    eng = _engine(c, gd=False, lane_node=False)
    lib = eng._lib
    on = C.c_int32(-7)
    try:
        assert lib.ldpc_hip_bp_get_decimation_lane_node(eng._h, C.byref(on)) == 0 and on.value == 0
        assert lib.ldpc_hip_bp_set_decimation_lane_node(eng._h, 1) == 0
        assert lib.ldpc_hip_bp_get_decimation_lane_node(eng._h, C.byref(on)) == 0 and on.value == 1 and eng.decimation_lane_node is True
        assert lib.ldpc_hip_bp_set_decimation_lane_node(eng._h, 2) == -1 and b"must be 0 or 1" in lib.ldpc_hip_last_error()
        assert lib.ldpc_hip_bp_get_decimation_lane_node(eng._h, C.byref(on)) == 0 and on.value == 1, "a refused value leaves the switch as it was"
        assert lib.ldpc_hip_bp_set_decimation_lane_node(None, 1) == -1
        assert lib.ldpc_hip_bp_get_decimation_lane_node(None, C.byref(on)) == -1 and lib.ldpc_hip_bp_get_decimation_lane_node(eng._h, None) == -1
        # a setting of the handle, independent of the variant: it survives the decimation going on and off
        eng.set_decimation(3, 6, 25.0)
        route = C.c_int32(-1)
        assert lib.ldpc_hip_bp_decimation_route(eng._h, 70, C.byref(route)) == 0 and route.value in (3, 4)
        eng.set_decimation(None)
        assert eng.decimation_lane_node is True
        eng.set_decimation_lane_node(False)
        assert eng.decimation_lane_node is False
    finally:
        eng.close()


# ---- 9. above the engine ------------------------------------------------------------------------------------------------------------------------
def _no_zero_rows(c, want):
    keep = c["synd"].any(axis=1)  # (an all-zero row takes the decoder's host shortcut: converged, 0 iterations)
    return dict(c, synd=np.ascontiguousarray(c["synd"][keep])), gw.take(want, np.flatnonzero(keep))


def test_bpgd_decoder_with_lane_node():
    from ldpc_amd.bpgd_decoder import BpgdDecoder
    c, want = _no_zero_rows(gw.every_instantiation("hgp400"), gw.want_instantiation("hgp400"))
    early, late, never = gu.shows(want, gw.R)
    assert early > 0 and late > 0 and never > 0
    d = BpgdDecoder(c["h"], channel_probs=c["probs"], round_iters=gw.T, max_rounds=gw.R, freeze_llr=gw.C, ms_scaling_factor=c["alpha"], lane_node=True)
    assert d.route in ("bp_wave", "bp_wave_team")
    with launch_util.launch_log() as log:
        dec = d.decode_batch(c["synd"])
    _same((dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), want, "BpgdDecoder.decode_batch")
    assert len(launch_util.of(log, "bp_wave_gd_kernel")) == 1
    launch_util.assert_not_ran(log, *PLAIN_BP, *EDGE_GD)
    for row in (int(np.flatnonzero(~want[3])[0]), int(np.flatnonzero(want[4]["solved_round"] > 0)[0])):
        out = d.decode(c["synd"][row])
        _same((out[None, :], d.log_prob_ratios[None, :], np.array([d.iter]), np.array([d.converge])), tuple(x[row:row + 1] for x in want[:4]), f"BpgdDecoder.decode row {row}")
    off = BpgdDecoder(c["h"], channel_probs=c["probs"], round_iters=gw.T, max_rounds=gw.R, ms_scaling_factor=c["alpha"])
    assert off.route == "unavailable"
    with pytest.raises(NotImplementedError, match=OLD_SENTENCE):
        off.decode_batch(c["synd"])


def test_bposd_osd0_with_lane_node(oracle_built):
    """Rows with a solution: the restatement's.  Rows without: H x = s, and OSD-0 of the host oracle on the restatement's last posteriors."""
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    c, want = _no_zero_rows(gw.every_instantiation("hgp400"), gw.want_instantiation("hgp400"))
    dec, llr, it, cv = want[:4]
    orc = oracle_built.BpOracle(c["h"], error_channel=c["probs"], max_iter=12, bp_method="minimum_sum", ms_scaling_factor=c["alpha"])
    expect = dec.copy()
    for b in np.flatnonzero(~cv):
        expect[b] = orc.osdw(c["synd"][b], llr[b], 1, 0)[0]
    d = BpOsdDecoder(c["h"], error_channel=list(c["probs"]), max_iter=12, bp_method="minimum_sum", ms_scaling_factor=c["alpha"], osd_method="osd_0")
    d.decimation = dict(round_iters=gw.T, max_rounds=gw.R)
    d.decimation_lane_node = True
    with launch_util.launch_log() as log:
        got = d.decode_batch(c["synd"])
    _same((got, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), (expect, llr, it, cv), "BpOsdDecoder with the decimation")
    assert len(launch_util.of(log, "bp_wave_gd_kernel")) == 1
    hd = c["h"].toarray().astype(np.int64)
    left = np.flatnonzero(~cv)
    assert len(left) and np.array_equal((got[left].astype(np.int64) @ hd.T) & 1, c["synd"][left]), "an OSD row does not satisfy H x = s"


def test_the_monte_carlo_class_with_lane_node():
    """bb144 x 3 rounds, BPGD + OSD-0: the counts equal those of decoding the NumPy twin's shots through decode_b8 and counting on the host."""
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from test_dem_sampler_twin import unpack
    from test_gpu_dem_sampler import SEED, engine, model, twin
    check, obs, pri = model("bb144x3")
    gd = dict(round_iters=3, max_rounds=6)
    eng = engine(check, pri, obs)
    try:
        eng.set_osd(1, 0)
        eng.set_decimation_lane_node(True)
        eng.set_decimation(3, 6, 25.0)
        assert eng.decimation_route(3000) in ("bp_wave", "bp_wave_team")
        _, dets, true_obs = twin("bb144x3", False, 0)
        with launch_util.launch_log() as log:
            pred, _, iters, conv = eng.decode_b8(np.array(dets), with_osd=True)
        assert launch_util.of(log, "bp_wave_gd_kernel") in ([_name((8, 4), False)], [_name((8, 4), True)])
        launch_util.assert_not_ran(log, *PLAIN_BP, *EDGE_GD)
        synd = unpack(np.array(dets), check.shape[0])
        ref = gu.bpgd_restatement(check, np.clip(pri, 1e-9, 1 - 1e-9), synd, 3, 6, 25.0, 0.625, details=True)
        print(f"bb144x3: {gu.shows(ref, 6)}")
        assert ref[3].any() and (ref[4]["solved_round"] > 0).any()
        ref_iters = np.where(synd.any(axis=1), ref[2], 0)  # (decode_b8: all-zero rows take the shortcut -- converged, 0 iterations)
        assert np.array_equal(np.asarray(conv, bool), ref[3] | ~synd.any(axis=1)) and np.array_equal(np.asarray(iters), ref_iters), \
            "decode_b8 with the decimation: flags or iteration counts"
        want = (int(np.count_nonzero((pred != true_obs).any(axis=1))), int(np.count_nonzero(~np.asarray(conv, bool))))
        print(f"bb144x3 with the decimation + OSD-0: {want[0]} logical failures, {want[1]} rows left without a solution, of 3000")
        # the same shots through decode_batch (BP + OSD-0), the observables and both counts formed on the host
        dec, _, _, cv = eng.decode_batch(synd, osd0=True)
        host_pred = (np.asarray(dec).astype(np.int64) @ sp.csr_matrix(obs).toarray().astype(np.int64).T) & 1
        host = (int(np.count_nonzero((host_pred != np.asarray(true_obs)).any(axis=1))), int(np.count_nonzero(~np.asarray(cv, bool))))
        assert host == want, f"decode_batch and counting on the host: {host}, decode_b8: {want}"
    finally:
        eng.close()
    got = MonteCarloDemSimulation((check, obs, pri), target_run_count=3000, batch_size=1024, seed=SEED, max_iter=12, decimation=gd, decimation_lane_node=True).run()
    assert (got["fail_count"], got["bp_unconverged_count"]) == want


def test_the_switch_alone_leaves_a_sharded_decoder_decoding():
    """decimation_lane_node is read only while decimation is set: on a decoder sharded over GPUs (whose engine has no such setter, and which
    refuses decimation) setting it changes nothing about an ordinary decode."""
    from ldpc_amd.bp_decoder import BpDecoder
    c = gw.every_instantiation("ldpc64_58")
    kw = dict(error_channel=list(c["probs"]), max_iter=12, bp_method="minimum_sum", ms_scaling_factor=c["alpha"], input_vector_type="syndrome")
    want = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], 12, c["alpha"], np.float64)
    for more in (dict(device_ids=[0, 0]), {}):
        b = BpDecoder(c["h"], **kw, **more)
        b.decimation_lane_node = True
        dec = b.decode_batch(c["synd"])
        assert np.array_equal(dec, want[0]) and np.array_equal(np.asarray(b.converge_batch, bool), want[3]), more
    b = BpDecoder(c["h"], **kw, device_ids=[0, 0])
    b.decimation_lane_node = True
    b.decimation = dict(round_iters=3, max_rounds=6)
    with pytest.raises(NotImplementedError, match=r"decimation with device_ids"):
        b.decode_batch(c["synd"])


def test_close_frees_every_device_buffer():
    from ldpc_amd import _lib
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    c = gw.every_instantiation("hgp400")
    eng = _engine(c, gd=False)
    try:
        eng.decode_batch(c["synd"])
        eng.set_decimation(gw.T, gw.R, gw.C)
        eng.decode_batch(c["synd"])
        first = held()
        for _ in range(3):  # off and on again: the padded priors go and come back, nothing piles up
            eng.set_decimation(None)
            assert held() < first
            eng.set_decimation(gw.T, gw.R, gw.C)
            eng.decode_batch(c["synd"])
            assert held() == first
        eng.set_decimation_lane_node(False)
        assert held() < first, "switching the lane = node route off releases its padded priors"
        eng.set_decimation_lane_node(True)
        eng.decode_batch(c["synd"])
        assert held() == first
    finally:
        eng.close()
    assert held() == before, f"{held() - before} bytes of device buffers outlive the handle"
