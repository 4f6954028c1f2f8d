"""Relay-BP on the device (ldpc_hip_bp_set_relay) against the NumPy restatement (tests/relay_bp_util.py), bit for bit:
hard decisions, converge flags, total iteration counts and the bit patterns of the posteriors -- on the lane = edge relay kernels
(bp_edge_relay_kernel, bp_edge8_relay_kernel: every instantiation once) and on the per-pass leg loop (bp_spread_relay_init_kernel,
relay_select_kernel around the per-pass memory kernels), with the launch log showing which route ran; then what goes round them: one leg
against the memory decode, on / off / on, new channel probabilities, the decoder classes, BP + OSD-0, the detector-error-model loop, the
refusals of the C ABI, and that close() frees every buffer.

Every comparison on the edge_case codes first asserts ON THE RESTATEMENT'S OUTPUT that the batch holds a row without a solution, a row
stopped at stop_after, a row with fewer solutions, a row first solved after leg 0 (relay_bp_util.assert_shows_something) -- and, once per
kernel family, a row whose later solution replaced an earlier one."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import f32_util as fu
import ladder_util as lu
import launch_util
import mem_bp_util as mu
import relay_bp_util as ru
from oracle import bits_equal

pytestmark = pytest.mark.gpu

EDGE_RELAY = ("bp_edge_relay_kernel", "bp_edge8_relay_kernel")
LEG_LOOP = ("bp_spread_mem_init_kernel", "bp_spread_relay_init_kernel", "bp_spread_mem_bit_kernel", "bp_spread_mem_finish_kernel", "relay_select_kernel")
EDGE_MEM = ("bp_edge_mem_kernel", "bp_edge8_mem_kernel")
PER_PASS_PLAIN = ("bp_spread_init_kernel", "bp_spread_bit_kernel", "bp_spread_finish_kernel")
PLAIN_BP = tuple(k for k in lu.BP_DECODE_KERNELS if k not in ("bp_spread_check_kernel", "bp_spread_synd_kernel")) + ("bp_edge_rp_kernel", "bp_edge8_rp_kernel",
                                                                                                                     "bp_edge_f32_kernel", "bp_edge8_f32_kernel")


def _same(got, want, what):
    dec, llr, it, cv = got[:4]
    print(f"{what}: {int(np.count_nonzero(np.asarray(dec) != want[0]))} decisions, {int(np.count_nonzero(np.asarray(cv, bool) != want[3]))} flags, "
          f"{int(np.count_nonzero(np.asarray(it) != want[2]))} iteration counts differ, "
          f"{int(np.count_nonzero(np.ascontiguousarray(llr, np.float64).view(np.uint64) != np.ascontiguousarray(want[1]).view(np.uint64)))} posteriors differ in some bit")
    odd = np.flatnonzero((np.asarray(it) != want[2]) | (np.asarray(cv, bool) != want[3]))[:8]
    if len(odd):
        print(f"{what}: rows {odd.tolist()}: iterations {np.asarray(it)[odd].tolist()} for {want[2][odd].tolist()}, "
              f"flags {np.asarray(cv, bool)[odd].astype(int).tolist()} for {want[3][odd].astype(int).tolist()}")
    assert np.array_equal(np.asarray(dec), want[0]), f"{what}: hard decisions"
    assert np.array_equal(np.asarray(cv, bool), want[3]), f"{what}: converge flags"
    assert np.array_equal(np.asarray(it), want[2]), f"{what}: iteration counts"
    assert bits_equal(np.asarray(llr), want[1]), f"{what}: posteriors differ in some bit"


def _engine(c, relay=True, mode=None, switches=None, max_iter=12):
    from ldpc_amd.engine import HipBpEngine
    h = sp.csr_matrix(c["h"])
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], c["probs"], c.get("max_iter", max_iter), 1, c["alpha"])
    if mode is not None:
        eng.set_small_code_kernel(mode)
    for name, value in (switches or {}).items():
        eng.set_debug_switch(name, value)
    if relay:
        eng.set_relay(c["gamma"], c["leg_iters"], c["stop_after"])
    return eng


def _decode(c, mode=None, switches=None):
    eng = _engine(c, True, mode, switches)
    try:
        with launch_util.launch_log() as log:
            out = eng.decode_batch(c["synd"])
    finally:
        eng.close()
    return out, log


def _assert_leg_loop(log, legs):
    launch_util.assert_ran(log, "bp_spread_mem_init_kernel", "bp_spread_mem_bit_kernel", "bp_spread_mem_finish_kernel", "relay_select_kernel",
                           "bp_spread_check_kernel", "bp_spread_synd_kernel")
    assert log["relay_select_kernel"] == legs, f"relay_select_kernel ran {log['relay_select_kernel']} times for {legs} legs"
    if legs > 1:
        launch_util.assert_ran(log, "bp_spread_relay_init_kernel")
    launch_util.assert_not_ran(log, *PER_PASS_PLAIN, *EDGE_RELAY, *EDGE_MEM, *PLAIN_BP)


def _assert_edge_relay(log, name):
    launch_util.assert_resolved(log)
    assert launch_util.of(log, *EDGE_RELAY) == [name] and log[name] == 1, f"expected exactly {name}, once; the log has {sorted(log)}"
    launch_util.assert_ran(log, "edge_relay_table_kernel")
    launch_util.assert_not_ran(log, *LEG_LOOP, *EDGE_MEM, *PLAIN_BP, "bp_spread_check_kernel", "bp_spread_synd_kernel")


# ---- 1. the lane = edge relay kernels, and the same codes on the leg loop -------------------------------------------------------------------------
_EDGE_NAMES = {"surface5": "bp_edge_relay_kernel<1>", "bb144": "bp_edge8_relay_kernel<9, 3>", "hgp_hamming3": "bp_edge8_relay_kernel<3, 4>"}


def _edge_batch(code, rows):
    """(case, expected) of the first 300 rows, or of the B = 70 batch picked from them on the restatement's output."""
    full = ru.edge_case(code)
    want = ru.expected(code, full)
    if rows == 300:
        return full, want
    idx = ru.ragged_rows(want, full["stop_after"], rows)
    return dict(full, synd=np.ascontiguousarray(full["synd"][idx])), ru.take(want, idx)


@pytest.mark.parametrize("rows", [70, 300])
@pytest.mark.parametrize("code", list(_EDGE_NAMES))
def test_edge_kernels(code, rows):
    """6 legs of [12, 6, 6, 6, 6, 6] iterations, stop after 3 solutions, alpha 0.625; leg 0 at 0.125, legs 1 .. 5 drawn from [-0.24, 0.66]."""
    c, want = _edge_batch(code, rows)
    assert len(c["synd"]) == rows and tuple(c["leg_iters"]) == (12, 6, 6, 6, 6, 6) and c["stop_after"] == 3 and c["alpha"] == 0.625
    assert (c["gamma"][0] == 0.125).all() and c["gamma"][1:].min() >= -0.24 and c["gamma"][1:].max() <= 0.66
    # a later, lighter solution replaces an earlier one: once per kernel family at least (surface5: bp_edge_relay_kernel; the other two: bp_edge8_relay_kernel)
    ru.assert_shows_something(want, c["stop_after"], f"{code}/{rows}", need_replaced=True)
    got, log = _decode(c)
    _same(got, want, f"{code}/{rows} rows")
    _assert_edge_relay(log, _EDGE_NAMES[code])


@pytest.mark.parametrize("code", list(_EDGE_NAMES))
def test_edge_codes_on_the_leg_loop(code):
    """set_small_code_kernel(0): the same B = 70 batch through the per-pass leg loop, the same bits."""
    c, want = _edge_batch(code, 70)
    ru.assert_shows_something(want, c["stop_after"], f"{code} per pass")
    got, log = _decode(c, mode=0)
    _same(got, want, f"{code} with the on-chip kernels off")
    _assert_leg_loop(log, len(c["leg_iters"]))


def test_a_syndrome_byte_above_one_never_converges():
    """Bytes 2 and 3 in three rows of the bb144 batch: those rows run every leg to its end on both routes."""
    c, _ = _edge_batch("bb144", 70)
    synd = c["synd"].copy()
    synd[3, 5], synd[9, 0], synd[64, 71] = 2, 3, 2
    c = dict(c, synd=synd)
    want = ru.relay_restatement(c["h"], c["probs"], c["gamma"], c["leg_iters"], c["stop_after"], synd, c["alpha"])
    for b in (3, 9, 64):
        assert not want[3][b] and want[2][b] == sum(c["leg_iters"])
    assert want[3].any()
    for mode in (None, 0):
        got, log = _decode(c, mode=mode)
        _same(got, want, f"bytes > 1, mode {mode}")
        (_assert_edge_relay(log, "bp_edge8_relay_kernel<9, 3>") if mode is None else _assert_leg_loop(log, 6))


# ---- 2. the leg loop on codes the lane = edge kernels do not take, or with the on-chip kernels off -----------------------------------------------
def _loop_case(key):
    if key == "irregular600":
        c = fu.irregular_case()
        c = dict(c, gamma=ru.masked_strengths(c["probs"], 4), leg_iters=(8, 4, 4, 4), stop_after=2)
    else:
        c = fu.small_case(key, 0.625)
        c = dict(c, gamma=ru.masked_strengths(c["probs"], 4), leg_iters=(6, 3, 3, 3), stop_after=2)
    return c


@pytest.mark.parametrize("key", ["hamming3", "rep5", "irregular600"])
def test_leg_loop(key):
    """hamming3 and rep5 (B = 70; p = 0 / 1 / 0.5 / 1e-300 columns, strength 0 on the infinite priors; syndrome bytes 2 and 3) with the on-chip
    kernels off, and the irregular n = 600 code (B = 130, columns of up to 11 entries), which no on-chip kernel takes."""
    c = _loop_case(key)
    want = ru.expected(f"loop|{key}", c)
    d = want[4]
    print(f"{key}: {ru.shows(want, c['stop_after'])}")
    assert want[3].any() and not want[3].all(), f"{key}: rows with and without a solution"
    assert (want[2] > c["leg_iters"][0]).any(), f"{key}: no row runs a second leg"
    assert (d["nsol"] == c["stop_after"]).any(), f"{key}: no row stops at stop_after"
    got, log = _decode(c, mode=None if key == "irregular600" else 0)
    _same(got, want, key)
    _assert_leg_loop(log, len(c["leg_iters"]))


def test_leg_loop_scaling_factor_zero_counts_the_legs_iterations():
    """ms_scaling_factor 0: alpha = 1 - 2^-it with the LEG-LOCAL it, on both routes."""
    c, _ = _edge_batch("hgp_hamming3", 70)
    c = dict(c, alpha=0.0)
    want = ru.expected("hgp_hamming3|alpha0|70", c)
    assert want[3].any() and (want[2] > c["leg_iters"][0]).any()
    for mode in (None, 0):
        got, _ = _decode(c, mode=mode)
        _same(got, want, f"alpha 0, mode {mode}")


# ---- 3. every instantiation of both ladders once ---------------------------------------------------------------------------------------------------
_LADDER = [c for c in lu.EDGE_CASES if c.id.endswith("-percol") and c.build["m"] % 16 == 0] + \
          [c for c in lu.EDGE8_CASES if c.id.endswith("-percol") and c.build["m"] % 8 == 0 and c.build["m"] > 8]


def _relay_kernel_name(h):
    h = sp.csr_matrix(h)
    m, max_row, max_col = h.shape[0], int(np.diff(h.indptr).max()), int(np.asarray(h.sum(axis=0)).max())
    if max_row <= 4 and max_col <= 2:
        return f"bp_edge_relay_kernel<{lu.edge_rounds(m)}>"
    dc = 3 if max_col <= 3 else 4
    return f"bp_edge8_relay_kernel<{lu.edge8_rounds(m, dc)}, {dc}>"


def test_the_ladder_names_every_instantiation_once():
    names = sorted(_relay_kernel_name(lu.inputs(c.id)[0]) for c in _LADDER)
    want = sorted([f"bp_edge_relay_kernel<{r}>" for r in range(1, 17)] + [f"bp_edge8_relay_kernel<{r}, {dc}>" for dc in (3, 4) for r in lu.EDGE8_ROUNDS[dc]])
    assert names == want


@pytest.mark.parametrize("case", _LADDER, ids=[c.id for c in _LADDER])
def test_every_instantiation(case):
    """3 legs of [5, 3, 3] iterations, stop after 2, B = 70: rows with and without a solution, and rows that run more than one leg."""
    h, probs, synd = lu.inputs(case.id)
    c = dict(h=h, probs=np.array(probs), synd=np.ascontiguousarray(synd[:70]), alpha=case.alpha, gamma=ru.masked_strengths(probs, 3), leg_iters=(5, 3, 3), stop_after=2)
    want = ru.relay_restatement(c["h"], c["probs"], c["gamma"], c["leg_iters"], c["stop_after"], c["synd"], c["alpha"])
    assert want[3].any() and not want[3].all() and (want[2] > 5).any(), case.id
    eng = _engine(c, mode=case.mode)
    try:
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
    finally:
        eng.close()
    _same(got, want, case.id)
    _assert_edge_relay(log, _relay_kernel_name(h))


# ---- 4. one leg is the memory decode; on, off, on again; new channel probabilities -------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, 0], ids=["edge", "per-pass"])
def test_one_leg_is_the_memory_decode(mode):
    """One leg of max_iter iterations, stop after 1: the memory decode of the same handle parameters, and the memory restatement, bit for bit."""
    full = mu.edge_case("bb144")
    c = mu.first_rows(full, 70)
    g = mu.drawn_gamma(c["h"].shape[1], 7)
    want = tuple(x[:70] for x in mu.expected("bb144|drawn", full, g))
    mu.assert_shows_something(want, tuple(x[:70] for x in mu.plain("bb144", full)), c["max_iter"], "bb144/drawn")
    eng = _engine(c, relay=False, mode=mode)
    try:
        eng.set_memory(g)
        mem = eng.decode_batch(c["synd"])
        eng.set_memory(None)
        eng.set_relay(g[None, :], [c["max_iter"]], 1)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
    finally:
        eng.close()
    _same(got, want, "one leg against the memory restatement")
    _same(got, tuple(np.asarray(x) if k != 3 else np.asarray(x, bool) for k, x in enumerate(mem)), "one leg against the memory decode")
    (_assert_edge_relay(log, "bp_edge8_relay_kernel<9, 3>") if mode is None else _assert_leg_loop(log, 1))


@pytest.mark.parametrize("mode", [None, 0], ids=["edge", "per-pass"])
def test_on_off_on_again(mode):
    c, want1 = _edge_batch("bb144", 70)
    c2 = dict(c, gamma=ru.drawn_strengths(c["h"].shape[1], 4, seed=8), leg_iters=(9, 5, 5, 5), stop_after=2)
    want2 = ru.expected("bb144|second|70", c2)
    assert want2[3].any() and not want2[3].all() and not bits_equal(want1[1], want2[1])
    plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], 12, c["alpha"], np.float64)
    eng = _engine(c, relay=False, mode=mode)
    try:
        assert eng.relay is None
        with launch_util.launch_log() as log0:
            got = eng.decode_batch(c["synd"])
        _same(got, plain, "before the relay")
        launch_util.assert_not_ran(log0, *EDGE_RELAY, *LEG_LOOP)
        eng.set_relay(c["gamma"], c["leg_iters"], c["stop_after"])
        g, li, stop = eng.relay
        assert np.array_equal(g, c["gamma"]) and li.tolist() == list(c["leg_iters"]) and stop == c["stop_after"]
        _same(eng.decode_batch(c["synd"]), want1, "first relay")
        eng.set_relay(None)
        assert eng.relay is None
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, plain, "relay off again")
        assert log == log0, f"with the relay off the handle launches {sorted(log.items())}, before it was ever set {sorted(log0.items())}"
        eng.set_relay(c2["gamma"], c2["leg_iters"], c2["stop_after"])
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, want2, "second relay")
        (_assert_edge_relay(log, "bp_edge8_relay_kernel<9, 3>") if mode is None else _assert_leg_loop(log, 4))
    finally:
        eng.close()


@pytest.mark.parametrize("mode", [None, 0], ids=["edge", "per-pass"])
def test_channel_probabilities_set_after_the_relay_are_followed(mode):
    c = _loop_case("hamming3")
    other = dict(c, probs=np.array([0.03, 0.2, 0.45, 0.07, 0.11, 0.3, 0.06]))
    other["gamma"] = ru.drawn_strengths(7, 4, seed=9)
    want = ru.expected("loop|hamming3_other", other)
    assert want[3].any() and not want[3].all()
    eng = _engine(c, mode=mode)
    try:
        _same(eng.decode_batch(c["synd"]), ru.expected("loop|hamming3", c), "before")
        eng.set_relay(other["gamma"], other["leg_iters"], other["stop_after"])  # (nonzero now on what are p = 0 / 1 columns until the next line)
        eng.set_channel(other["probs"])
        _same(eng.decode_batch(c["synd"]), want, "after set_channel")
    finally:
        eng.close()


# ---- 5. the decoder classes, BP + OSD-0, the detector-error-model loop ------------------------------------------------------------------------------
def test_relay_bp_decoder():
    from ldpc_amd.relay_decoder import RelayBpDecoder
    c, want = _edge_batch("bb144", 70)
    d = RelayBpDecoder(c["h"], channel_probs=c["probs"], ms_scaling_factor=c["alpha"], strengths=c["gamma"], pre_iter=12, set_max_iter=6, stop_nconv=3)
    assert np.array_equal(d.strengths, c["gamma"]) and d.leg_iters.tolist() == [12, 6, 6, 6, 6, 6]
    assert c["synd"].any(axis=1).all(), "no all-zero row: nothing takes the host shortcut"
    with launch_util.launch_log() as log:
        dec = d.decode_batch(c["synd"])
    _same((dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), want, "RelayBpDecoder.decode_batch")
    _assert_edge_relay(log, "bp_edge8_relay_kernel<9, 3>")
    for row in (int(np.flatnonzero(~want[3])[0]), int(np.flatnonzero(want[4]["replaced"] > 0)[0])):
        out = d.decode(c["synd"][row])
        _same((out[None, :], d.log_prob_ratios[None, :], np.array([d.iter]), np.array([d.converge])), tuple(x[row:row + 1] for x in want[:4]), f"RelayBpDecoder.decode row {row}")
    # drawn at construction, as documented; update_channel_probs is followed
    d2 = RelayBpDecoder(c["h"], error_rate=0.2, gamma0=0.125, pre_iter=12, num_sets=5, set_max_iter=6, stop_nconv=3, ms_scaling_factor=c["alpha"], seed=7)
    assert np.array_equal(d2.strengths[1:], np.random.default_rng(7).uniform(-0.24, 0.66, (5, c["h"].shape[1]))) and (d2.strengths[0] == 0.125).all()
    assert np.array_equal(d2.strengths, c["gamma"])
    d2.update_channel_probs(c["probs"])
    dec = d2.decode_batch(c["synd"])
    _same((dec, d2.log_prob_ratios_batch, d2.iter_batch, d2.converge_batch), want, "RelayBpDecoder after update_channel_probs")


def test_bposd_osd0_with_the_relay(oracle_built):
    """Rows with a solution: the restatement's.  Rows without: H x = s, and OSD-0 of the host oracle on the restatement's posteriors."""
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    c, want = _edge_batch("bb144", 70)
    dec, llr, it, cv = want[:4]
    orc = oracle_built.BpOracle(c["h"], error_channel=c["probs"], max_iter=12, bp_method="minimum_sum", ms_scaling_factor=c["alpha"])
    expect = dec.copy()
    for b in np.flatnonzero(~cv):
        expect[b] = orc.osdw(c["synd"][b], llr[b], 1, 0)[0]
    d = BpOsdDecoder(c["h"], error_channel=list(c["probs"]), max_iter=12, bp_method="minimum_sum", ms_scaling_factor=c["alpha"], osd_method="osd_0")
    d.relay = dict(strengths=c["gamma"], pre_iter=12, set_max_iter=6, stop_nconv=3)
    with launch_util.launch_log() as log:
        got = d.decode_batch(c["synd"])
    _same((got, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), (expect, llr, it, cv), "BpOsdDecoder with the relay")
    _assert_edge_relay(log, "bp_edge8_relay_kernel<9, 3>")
    hd = c["h"].toarray().astype(np.int64)
    left = np.flatnonzero(~cv)
    assert len(left) and np.array_equal((got[left].astype(np.int64) @ hd.T) & 1, c["synd"][left]), "an OSD row does not satisfy H x = s"
    d.osd_method = "osd_cs"
    d.osd_order = 3
    with pytest.raises(NotImplementedError, match="relay with osd_method='OSD_CS'"):
        d.decode_batch(c["synd"])


def test_simulate_b8_and_the_monte_carlo_class_with_the_relay():
    """hamming3 x 7 rounds, Relay-BP + OSD-0: both counters equal twin -> relay decode_b8 -> compare, for chunks 3000 and 64; the decode_b8
    flags and iteration counts are the restatement's."""
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from test_dem_sampler_twin import unpack
    from test_gpu_dem_sampler import SEED, engine, model, twin
    check, obs, pri = model("hamming3x7")
    n = check.shape[1]
    relay = dict(gamma0=0.125, pre_iter=8, num_sets=3, set_max_iter=4, stop_nconv=2, seed=11)
    from ldpc_amd.relay_decoder import relay_schedule
    g, li, stop = relay_schedule(n, **relay)
    eng = engine(check, pri, obs)
    try:
        eng.set_osd(1, 0)
        eng.set_relay(g, li, stop)
        _, dets, true_obs = twin("hamming3x7", False, 0)
        with launch_util.launch_log() as log:
            pred, _, iters, conv = eng.decode_b8(np.array(dets), with_osd=True)
        launch_util.assert_ran(log, "relay_select_kernel") if not launch_util.of(log, *EDGE_RELAY) else None
        launch_util.assert_not_ran(log, *PLAIN_BP, *EDGE_MEM)
        synd = unpack(np.array(dets), check.shape[0])
        ref = ru.relay_restatement(check, np.clip(pri, 1e-9, 1 - 1e-9), g, li, stop, synd, 0.625)
        assert ref[3].any() and not ref[3].all() and (ref[2] > 8).any()
        ref_iters = np.where(synd.any(axis=1), ref[2], 0)  # (decode_b8: all-zero rows take the shortcut -- converged, 0 iterations)
        assert np.array_equal(np.asarray(conv, bool), ref[3] | ~synd.any(axis=1)) and np.array_equal(np.asarray(iters), ref_iters), \
            "decode_b8 with the relay: flags or iteration counts"
        want = (int(np.count_nonzero((pred != true_obs).any(axis=1))), int(np.count_nonzero(~np.asarray(conv, bool))))
        print(f"hamming3x7 with the relay + OSD-0: {want[0]} logical failures, {want[1]} rows left without a solution, of 3000")
        assert want[1] > 0
        for chunk in (3000, 64):
            assert eng.simulate_b8(SEED, 0, 3000, chunk=chunk, with_osd=True) == want, f"chunk {chunk}"
    finally:
        eng.close()
    got = MonteCarloDemSimulation((check, obs, pri), target_run_count=3000, batch_size=1024, seed=SEED, max_iter=12, relay=relay).run()
    assert (got["fail_count"], got["bp_unconverged_count"]) == want


# ---- 6. the C ABI: refusals, buffers ------------------------------------------------------------------------------------------------------------
def test_cabi_refusals():
    from ldpc_amd import _lib
    c = _loop_case("hamming3")
    n = c["h"].shape[1]
    g = c["gamma"]
    li = np.array(c["leg_iters"], np.int32)
    eng = _engine(c)
    lib = eng._lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        # the setter: -1 (LDPC_HIP_ERR_INVALID), and what it held stays
        for bad in (1.0, -1.5, float("nan"), float("inf")):
            v = g.copy()
            v[2, 3] = bad
            assert lib.ldpc_hip_bp_set_relay(eng._h, 4, vp(v), vp(li), 2) == -1
            assert b"memory strength 3 of leg 2" in lib.ldpc_hip_last_error() and b"[-1, 1)" in lib.ldpc_hip_last_error()
            with pytest.raises(ValueError, match=r"memory strength 3 of leg 2"):
                eng.set_relay(v, li, 2)
        zero = li.copy()
        zero[1] = 0
        assert lib.ldpc_hip_bp_set_relay(eng._h, 4, vp(g), vp(zero), 2) == -1 and b"leg 1" in lib.ldpc_hip_last_error()
        assert lib.ldpc_hip_bp_set_relay(eng._h, 4, vp(g), vp(li), 0) == -1 and b"stop_after" in lib.ldpc_hip_last_error()
        assert lib.ldpc_hip_bp_set_relay(eng._h, 4, vp(g), None, 2) == -1
        assert lib.ldpc_hip_bp_set_relay(None, 0, None, None, 0) == -1 and lib.ldpc_hip_bp_get_relay(None, None, None, None, None) == -1
        got = eng.relay
        assert np.array_equal(got[0], g) and got[1].tolist() == li.tolist() and got[2] == 2
        # relay and memory exclude each other, either way round, each naming what to switch off
        assert lib.ldpc_hip_bp_set_memory(eng._h, vp(np.zeros(n))) == -4 and b"ldpc_hip_bp_set_relay(h, 0" in lib.ldpc_hip_last_error()
        eng.set_relay(None)
        eng.set_memory(np.zeros(n))
        assert lib.ldpc_hip_bp_set_relay(eng._h, 4, vp(g), vp(li), 2) == -4 and b"ldpc_hip_bp_set_memory(h, NULL)" in lib.ldpc_hip_last_error()
        eng.set_memory(None)
        eng.set_relay(g, li, 2)
        # the modes, each with its message, nothing launched
        probs_rows = np.tile(np.clip(c["probs"], 0.01, 0.99), (len(c["synd"]), 1))
        with launch_util.launch_log() as log:
            eng.set_params(12, 0, 1.0)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: Relay-BP: product-sum"):
                eng.decode_batch(c["synd"])
            eng.set_params(12, 1, 0.625)
            for schedule in ("serial", "serial_relative"):
                eng.set_schedule(schedule)
                with pytest.raises(_lib.LdpcHipError, match=r"error -4: Relay-BP: the serial schedules"):
                    eng.decode_batch(c["synd"])
            eng.set_schedule("parallel")
            eng.set_random_serial(True, 5)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: Relay-BP: the serial schedules"):
                eng.decode_batch(c["synd"])
            eng.set_random_serial(False, 5)
            eng.set_message_dtype("float32")
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: Relay-BP: float32 messages"):
                eng.decode_batch(c["synd"])
            eng.set_message_dtype("float64")
            for osd0 in (False, True):
                with pytest.raises(_lib.LdpcHipError, match=r"error -4: Relay-BP: per-row channel probabilities"):
                    eng.decode_batch(c["synd"], osd0=osd0, channel_probs=probs_rows)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: Relay-BP: soft-syndrome"):
                eng.soft_info_decode_batch(np.ones((2, 3)), np.inf, 2.0)
            for method in (2, 3):
                eng.set_osd(method, 2)
                with pytest.raises(_lib.LdpcHipError, match=r"error -4: Relay-BP: OSD-E and OSD-CS"):
                    eng.decode_batch(c["synd"], osd=True)
            eng.set_osd(1, 0)
            # a nonzero strength in one leg on the p = 0 column: refused at decode time, naming what it needs
            v = g.copy()
            assert c["probs"][0] == 0.0 and (v[:, 0] == 0.0).all()
            v[3, 0] = 0.2
            eng.set_relay(v, li, 2)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: Relay-BP: column 0 .*strictly between 0 and 1"):
                eng.decode_batch(c["synd"])
            with pytest.raises(_lib.LdpcHipError, match=r"strictly between 0 and 1"):
                eng.decode_batch(c["synd"], osd=True)
        assert not log, f"a refused decode launched something: {sorted(log)}"
        # ... and the handle still decodes
        eng.set_relay(g, li, 2)
        _same(eng.decode_batch(c["synd"]), ru.expected("loop|hamming3", c), "after the refusals")
    finally:
        eng.close()


def test_close_frees_every_device_buffer():
    from ldpc_amd import _lib
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    c, _ = _edge_batch("bb144", 70)
    for case, mode in ((c, None), (c, 0), (_loop_case("irregular600"), None)):
        eng = _engine(case, mode=mode)
        try:
            eng.decode_batch(case["synd"])
            with_relay = held()
            eng.set_relay(None)
            assert held() < with_relay, "switching the relay off releases its tables and leg buffers"
            eng.decode_batch(case["synd"])
            eng.set_relay(case["gamma"], case["leg_iters"], case["stop_after"])
            eng.set_osd(1, 0)
            eng.decode_batch(case["synd"], osd=True)
            during = held()
        finally:
            eng.close()
        after = held()
        print(f"Relay-BP: device buffer bytes before {before}, with the engine {during}, after close {after}")
        assert during > before and after == before, f"{after - before} bytes of device buffers outlive the handle"
