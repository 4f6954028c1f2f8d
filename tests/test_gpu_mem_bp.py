"""Memory min-sum BP on the device (ldpc_hip_bp_set_memory) against the NumPy restatement (tests/mem_bp_util.py), bit
for bit: hard decisions, converge flags, iteration counts and the bit patterns of the posteriors -- on the per-pass memory kernels
(bp_spread_mem_*), on the lane = edge memory kernels (bp_edge_mem_kernel, bp_edge8_mem_kernel: every instantiation once), with the launch
log showing which family ran; then what goes round them: strength zero, on / off / on, new channel probabilities, BP + OSD, the
detector-error-model loop, the refusals of the C ABI, and that close() frees every buffer.

Every comparison first asserts ON THE RESTATEMENT'S OUTPUT that the batch holds a row that converges before max_iter, a row that does not
converge, and a row that differs from the plain decode (mem_bp_util.assert_shows_something)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import f32_util as fu
import ladder_util as lu
import launch_util
import mem_bp_util as mu
from oracle import bits_equal

pytestmark = pytest.mark.gpu

PER_PASS_MEM = ("bp_spread_mem_init_kernel", "bp_spread_mem_bit_kernel", "bp_spread_mem_finish_kernel")
PER_PASS_PLAIN = ("bp_spread_init_kernel", "bp_spread_bit_kernel", "bp_spread_finish_kernel")  # (the check and syndrome kernels see no prior: shared)
EDGE_MEM = ("bp_edge_mem_kernel", "bp_edge8_mem_kernel")
# every plain BP decode kernel but the two per-pass kernels the memory route shares
PLAIN_BP = tuple(k for k in lu.BP_DECODE_KERNELS if k not in ("bp_spread_check_kernel", "bp_spread_synd_kernel")) + ("bp_edge_rp_kernel", "bp_edge8_rp_kernel",
                                                                                                                     "bp_edge_f32_kernel", "bp_edge8_f32_kernel")


def _same(got, want, what):
    dec, llr, it, cv = got
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


def _engine(c, gamma=None, mode=None, switches=None):
    from ldpc_amd.engine import HipBpEngine
    h = sp.csr_matrix(c["h"])
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], c["probs"], c["max_iter"], 1, c["alpha"])
    if mode is not None:
        eng.set_small_code_kernel(mode)
    for name, value in (switches or {}).items():
        eng.set_debug_switch(name, value)
    if gamma is not None:
        eng.set_memory(gamma)
    return eng


def _decode(c, gamma, mode=None, switches=None):
    eng = _engine(c, gamma, mode, switches)
    try:
        with launch_util.launch_log() as log:
            out = eng.decode_batch(c["synd"])
    finally:
        eng.close()
    return out, log


def _assert_per_pass_mem(log):
    launch_util.assert_ran(log, *PER_PASS_MEM, "bp_spread_check_kernel", "bp_spread_synd_kernel")
    launch_util.assert_not_ran(log, *PER_PASS_PLAIN, *EDGE_MEM, *PLAIN_BP)


def _assert_edge_mem(log, name):
    launch_util.assert_resolved(log)
    assert launch_util.of(log, *EDGE_MEM) == [name] and log[name] == 1, f"expected exactly {name}, once; the log has {sorted(log)}"
    launch_util.assert_not_ran(log, *PER_PASS_MEM, *PLAIN_BP, "bp_spread_check_kernel", "bp_spread_synd_kernel")


def _checked(key, c, gamma):
    """The restatement of (case, gamma), after asserting that it shows something."""
    want = mu.expected(key, c, gamma)
    mu.assert_shows_something(want, mu.plain(key.split("|")[0], c), c["max_iter"], key)
    return want


# ---- 1. the per-pass memory kernels ------------------------------------------------------------------------------------------------------------
def _small(code, alpha):
    c = fu.small_case(code, alpha)
    return c, mu.mixed_gamma(c["probs"])


@pytest.mark.parametrize("alpha", [0.625, 0.0])
@pytest.mark.parametrize("code", ["hamming3", "rep5"])
def test_per_pass_small_codes(code, alpha):
    """B = 70 (64 + 6), p = 0 / 1 / 0.5 / 1e-300 columns (strength 0 on the infinite priors, nonzero on the zero prior), syndrome bytes 2 and 3;
    mode 0: these codes would otherwise go to the lane = edge kernels."""
    c, g = _small(code, alpha)
    assert (g[np.isin(c["probs"], (0.0, 1.0))] == 0).all() and (g[c["probs"] == 0.5] != 0).all() and (g < 0).any() and (g > 0).any()
    want = _checked(f"{code}_a{alpha}|mixed", c, g)
    got, log = _decode(c, g, mode=0)
    _same(got, want, f"{code} a = {alpha}")
    _assert_per_pass_mem(log)


def test_per_pass_irregular_code():
    """B = 130, rows up to 16 entries, columns of up to 11: the bit kernel's column path through memory (d > DC = 8) beside the one in registers."""
    c = fu.irregular_case()
    cols = np.asarray(sp.csr_matrix(c["h"]).sum(axis=0)).ravel()
    assert cols.max() > 8 and cols.min() <= 4
    g = mu.mixed_gamma(c["probs"])
    want = _checked("irregular600|mixed", c, g)
    got, log = _decode(c, g)
    _same(got, want, "irregular600")
    _assert_per_pass_mem(log)
    launch_util.assert_ran(log, "bp_spread_mem_bit_kernel<8, 0>", "bp_spread_check_kernel<1, 0, 16, 0, false>")


def test_per_pass_heavy_rows():
    """Rows of 20 and 17 entries (the check kernel's sweeps through memory) under the memory bit kernel."""
    c = fu.heavy_rows_case()
    g = mu.mixed_gamma(c["probs"])
    want = _checked("heavy_rows|mixed", c, g)
    got, log = _decode(c, g, mode=0)
    _same(got, want, "heavy rows")
    _assert_per_pass_mem(log)


@pytest.mark.parametrize("switches", [{"SPREAD_NODES": 1}, {"SPREAD_NODES": 16}, {"SPREAD_NT": 1}], ids=["nodes1", "nodes16", "nt"])
@pytest.mark.parametrize("key", ["hamming3", "irregular600"])
def test_per_pass_under_switches(key, switches):
    c, g = _small("hamming3", 0.625) if key == "hamming3" else (fu.irregular_case(), mu.mixed_gamma(fu.irregular_case()["probs"]))
    want = _checked(f"{'hamming3_a0.625' if key == 'hamming3' else key}|mixed", c, g)
    got, log = _decode(c, g, mode=0, switches=switches)
    _same(got, want, f"{key} under {switches}")
    _assert_per_pass_mem(log)
    if "SPREAD_NT" in switches:
        launch_util.assert_ran(log, "bp_spread_mem_bit_kernel<4, 1>" if key == "hamming3" else "bp_spread_mem_bit_kernel<8, 1>")


# ---- 2. the lane = edge memory kernels ---------------------------------------------------------------------------------------------------------
def _edge_kernel_name(h):
    h = sp.csr_matrix(h)
    m, max_row, max_col = h.shape[0], int(np.diff(h.indptr).max()), int(np.asarray(h.sum(axis=0)).max())
    if max_row <= 4 and max_col <= 2:
        return f"bp_edge_mem_kernel<{lu.edge_rounds(m)}>"
    dc = 3 if max_col <= 3 else 4
    return f"bp_edge8_mem_kernel<{lu.edge8_rounds(m, dc)}, {dc}>"


_EDGE_NAMES = {"surface5": "bp_edge_mem_kernel<1>", "bb144": "bp_edge8_mem_kernel<9, 3>", "hgp_hamming3": "bp_edge8_mem_kernel<3, 4>"}


def _edge_gamma(code, which):
    n = mu.edge_case(code)["h"].shape[1]
    return np.full(n, 0.35) if which == "scalar" else mu.drawn_gamma(n, 7)


@pytest.mark.parametrize("which", ["scalar", "drawn"])
@pytest.mark.parametrize("rows", [70, 3000])
@pytest.mark.parametrize("code", list(_EDGE_NAMES))
def test_edge_kernels(code, rows, which):
    """B = 70, and B = 3000 through the pooled work counters; max_iter 12; one strength everywhere, and per-bit strengths from [-0.24, 0.66]."""
    full = mu.edge_case(code)
    assert _edge_kernel_name(full["h"]) == _EDGE_NAMES[code]
    g = _edge_gamma(code, which)
    want_full = mu.expected(f"{code}|{which}", full, g)
    c = mu.first_rows(full, rows)
    want = tuple(x[:rows] for x in want_full)
    mu.assert_shows_something(want, tuple(x[:rows] for x in mu.plain(code, full)), c["max_iter"], f"{code}/{which}/{rows}")
    got, log = _decode(c, g)
    _same(got, want, f"{code}/{which}/{rows} rows")
    _assert_edge_mem(log, _EDGE_NAMES[code])


@pytest.mark.parametrize("code", list(_EDGE_NAMES))
def test_edge_codes_on_the_per_pass_kernels(code):
    """set_small_code_kernel(0): the same batch through the per-pass memory kernels, the same bits."""
    full = mu.edge_case(code)
    g = _edge_gamma(code, "drawn")
    c = mu.first_rows(full, 70)
    want = tuple(x[:70] for x in mu.expected(f"{code}|drawn", full, g))
    mu.assert_shows_something(want, tuple(x[:70] for x in mu.plain(code, full)), c["max_iter"], code)
    got, log = _decode(c, g, mode=0)
    _same(got, want, f"{code} with the on-chip kernels off")
    _assert_per_pass_mem(log)


# one synthetic code per instantiation of both ladders (tests/ladder_util.py: the per-column-prior case at the upper end of every R), B = 70
_LADDER = [c for c in lu.EDGE_CASES if c.id.endswith("-percol") and c.build["m"] % 16 == 0] + \
          [c for c in lu.EDGE8_CASES if c.id.endswith("-percol") and c.build["m"] % 8 == 0 and c.build["m"] > 8]


def test_the_ladder_names_every_instantiation_once():
    names = sorted(_edge_kernel_name(lu.inputs(c.id)[0]) for c in _LADDER)
    want = sorted([f"bp_edge_mem_kernel<{r}>" for r in range(1, 17)] + [f"bp_edge8_mem_kernel<{r}, {dc}>" for dc in (3, 4) for r in lu.EDGE8_ROUNDS[dc]])
    assert names == want


@pytest.mark.parametrize("case", _LADDER, ids=[c.id for c in _LADDER])
def test_every_instantiation(case):
    h, probs, synd = lu.inputs(case.id)
    c = dict(h=h, probs=np.array(probs), synd=np.ascontiguousarray(synd[:70]), max_iter=lu.MAX_ITER, alpha=case.alpha)
    g = mu.mixed_gamma(c["probs"])
    want = mu.min_sum_memory_restatement(c["h"], c["probs"], g, c["synd"], c["max_iter"], c["alpha"])
    plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], c["max_iter"], c["alpha"], np.float64)
    mu.assert_shows_something(want, plain, c["max_iter"], case.id)
    got, log = _decode(c, g, mode=case.mode)
    _same(got, want, case.id)
    _assert_edge_mem(log, _edge_kernel_name(h))


# ---- 3. strength zero; on, off, on again; new channel probabilities ------------------------------------------------------------------------------
def _zero_case(key):
    return fu.small_case("hamming3", 0.625) if key == "hamming3" else mu.first_rows(mu.edge_case(key), 70)


@pytest.mark.parametrize("key", ["hamming3", "bb144", "surface5"])
def test_strength_zero_is_the_plain_decode(key):
    """Memory ON with an all-zero vector: the plain FP64 decode of the same handle, bit for bit (the p = 0, 1, 0.5, 1e-300 columns of hamming3
    included) -- through the memory kernels."""
    c = _zero_case(key)
    eng = _engine(c)
    try:
        with launch_util.launch_log() as log0:
            plain = eng.decode_batch(c["synd"])
        launch_util.assert_not_ran(log0, *EDGE_MEM, *PER_PASS_MEM)
        eng.set_memory(np.zeros(c["h"].shape[1]))
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, tuple(np.asarray(x) if k != 3 else np.asarray(x, bool) for k, x in enumerate(plain)), f"{key}: strength 0 against the plain decode")
        _assert_edge_mem(log, {"hamming3": "bp_edge8_mem_kernel<2, 3>", "bb144": "bp_edge8_mem_kernel<9, 3>", "surface5": "bp_edge_mem_kernel<1>"}[key])
        eng.set_small_code_kernel(0)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, tuple(np.asarray(x) if k != 3 else np.asarray(x, bool) for k, x in enumerate(plain)), f"{key}: strength 0 per pass against the plain decode")
        _assert_per_pass_mem(log)
    finally:
        eng.close()
    want = mu.plain(key if key != "hamming3" else "hamming3_a0.625", c if key == "hamming3" else mu.edge_case(key))
    _same(plain, tuple(x[:70] for x in want), f"{key}: the plain decode against the plain restatement")
    assert want[3][:70].any() and not want[3][:70].all()


@pytest.mark.parametrize("mode", [None, 0], ids=["edge", "per-pass"])
def test_on_off_on_again(mode):
    full = mu.edge_case("bb144")
    c = mu.first_rows(full, 70)
    g1, g2 = _edge_gamma("bb144", "scalar"), _edge_gamma("bb144", "drawn")
    want1 = tuple(x[:70] for x in mu.expected("bb144|scalar", full, g1))
    want2 = tuple(x[:70] for x in mu.expected("bb144|drawn", full, g2))
    plain = tuple(x[:70] for x in mu.plain("bb144", full))
    mu.assert_shows_something(want1, plain, c["max_iter"], "bb144/scalar")
    mu.assert_shows_something(want2, plain, c["max_iter"], "bb144/drawn")
    assert not bits_equal(want1[1], want2[1])
    eng = _engine(c, mode=mode)
    try:
        assert eng.memory() is None
        eng.set_memory(g1)
        assert np.array_equal(eng.memory(), g1)
        _same(eng.decode_batch(c["synd"]), want1, "first vector")
        eng.set_memory(None)
        assert eng.memory() is None
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, plain, "memory off again")
        launch_util.assert_not_ran(log, *EDGE_MEM, *PER_PASS_MEM)
        launch_util.assert_ran(log, "bp_edge8_kernel<9, 3, true>" if mode is None else "bp_spread_bit_kernel")
        eng.set_memory(g2)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, want2, "second vector")
        (_assert_edge_mem(log, "bp_edge8_mem_kernel<9, 3>") if mode is None else _assert_per_pass_mem(log))
    finally:
        eng.close()


@pytest.mark.parametrize("mode", [None, 0], ids=["edge", "per-pass"])
def test_channel_probabilities_set_after_the_memory_are_followed(mode):
    c, g = _small("hamming3", 0.625)
    other = dict(c, probs=np.array([0.03, 0.2, 0.45, 0.07, 0.11, 0.3, 0.06]))
    g_other = mu.mixed_gamma(other["probs"])
    want = mu.expected("hamming3_other|mixed", other, g_other)
    mu.assert_shows_something(want, mu.plain("hamming3_other", other), other["max_iter"], "hamming3 with other probabilities")
    eng = _engine(c, g, mode=mode)
    try:
        _same(eng.decode_batch(c["synd"]), _checked("hamming3_a0.625|mixed", c, g), "before")
        eng.set_memory(g_other)  # (nonzero now on what are p = 0 / 1 columns until the next line: refused only at decode time)
        eng.set_channel(other["probs"])
        _same(eng.decode_batch(c["synd"]), want, "after set_channel")
    finally:
        eng.close()


def test_decoder_classes():
    """BpDecoder.memory_strength: decode_batch and decode() through the batch kernels, with the all-zero shortcut of the host."""
    from ldpc_amd.bp_decoder import BpDecoder
    full = mu.edge_case("bb144")
    c = mu.first_rows(full, 70)
    want = tuple(x[:70] for x in mu.expected("bb144|scalar", full, _edge_gamma("bb144", "scalar")))
    mu.assert_shows_something(want, tuple(x[:70] for x in mu.plain("bb144", full)), c["max_iter"], "bb144/scalar")
    d = BpDecoder(c["h"], error_rate=float(c["probs"][0]), max_iter=c["max_iter"], bp_method="minimum_sum", ms_scaling_factor=c["alpha"], input_vector_type="syndrome")
    d.memory_strength = 0.35
    assert c["synd"].any(axis=1).all(), "no all-zero row: nothing takes the host shortcut"
    with launch_util.launch_log() as log:
        dec = d.decode_batch(c["synd"])
    _same((dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), want, "BpDecoder.decode_batch")
    _assert_edge_mem(log, "bp_edge8_mem_kernel<9, 3>")
    row = int(np.flatnonzero(~want[3])[0])
    with launch_util.launch_log() as log:
        out = d.decode(c["synd"][row])
    _same((out[None, :], d.log_prob_ratios[None, :], np.array([d.iter]), np.array([d.converge])), tuple(x[row:row + 1] for x in want), "BpDecoder.decode")
    _assert_edge_mem(log, "bp_edge8_mem_kernel<9, 3>")
    d.memory_strength = None
    plain = tuple(x[:70] for x in mu.plain("bb144", full))
    dec = d.decode_batch(c["synd"])
    _same((dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), plain, "BpDecoder.decode_batch with the memory off again")


# ---- 4. BP + OSD, the detector-error-model loop ---------------------------------------------------------------------------------------------------
def test_bposd_osd0_with_memory(oracle_built):
    """Rows BP converged: the restatement's.  Rows it left: H x = s, and OSD-0 of the host oracle on the restatement's posteriors."""
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    full = mu.edge_case("bb144")
    c = mu.first_rows(full, 70)
    dec, llr, it, cv = (x[:70] for x in mu.expected("bb144|scalar", full, _edge_gamma("bb144", "scalar")))
    mu.assert_shows_something((dec, llr, it, cv), tuple(x[:70] for x in mu.plain("bb144", full)), c["max_iter"], "bb144/scalar")
    orc = oracle_built.BpOracle(c["h"], error_channel=c["probs"], max_iter=c["max_iter"], bp_method="minimum_sum", ms_scaling_factor=c["alpha"])
    want = dec.copy()
    for b in np.flatnonzero(~cv):
        want[b] = orc.osdw(c["synd"][b], llr[b], 1, 0)[0]
    d = BpOsdDecoder(c["h"], error_rate=float(c["probs"][0]), max_iter=c["max_iter"], bp_method="minimum_sum", ms_scaling_factor=c["alpha"], osd_method="osd_0")
    d.memory_strength = 0.35
    with launch_util.launch_log() as log:
        got = d.decode_batch(c["synd"])
    _same((got, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), (want, llr, it, cv), "BpOsdDecoder with memory")
    _assert_edge_mem(log, "bp_edge8_mem_kernel<9, 3>")
    hd = c["h"].toarray().astype(np.int64)
    left = np.flatnonzero(~cv)
    assert len(left) and np.array_equal((got[left].astype(np.int64) @ hd.T) & 1, c["synd"][left]), "an OSD row does not satisfy H x = s"


def test_simulate_b8_and_the_monte_carlo_class_with_memory():
    """hamming3 x 7 rounds, min-sum 12 + OSD-0 with memory: both counters equal twin -> memory decode_b8 -> compare, for chunks 3000 and 64;
    the decode_b8 flags themselves are the restatement's."""
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from test_dem_sampler_twin import unpack
    from test_gpu_dem_sampler import SEED, engine, model, twin
    check, obs, pri = model("hamming3x7")
    n = check.shape[1]
    g = mu.drawn_gamma(n, 11)
    eng = engine(check, pri, obs)
    try:
        eng.set_osd(1, 0)
        eng.set_memory(g)
        _, dets, true_obs = twin("hamming3x7", False, 0)
        with launch_util.launch_log() as log:
            pred, _, iters, conv = eng.decode_b8(np.array(dets), with_osd=True)
        assert launch_util.of(log, *EDGE_MEM), f"no lane = edge memory kernel ran; the log has {sorted(log)}"
        launch_util.assert_not_ran(log, *PLAIN_BP, *PER_PASS_MEM)
        case = dict(h=check, probs=np.clip(pri, 1e-9, 1 - 1e-9), synd=unpack(np.array(dets), check.shape[0]), max_iter=12, alpha=0.625)
        ref = mu.expected("hamming3x7|drawn", case, g)
        ref_plain = mu.plain("hamming3x7", case)
        mu.assert_shows_something(ref, ref_plain, 12, "hamming3x7")
        ref_iters = np.where(case["synd"].any(axis=1), ref[2], 0)  # (decode_b8: all-zero rows take the shortcut -- converged, 0 iterations)
        assert np.array_equal(np.asarray(conv, bool), ref[3] | ~case["synd"].any(axis=1)) and np.array_equal(np.asarray(iters), ref_iters), \
            "decode_b8 with memory: flags or iteration counts"
        want = (int(np.count_nonzero((pred != true_obs).any(axis=1))), int(np.count_nonzero(~np.asarray(conv, bool))))
        print(f"hamming3x7 with memory, min-sum 12 + OSD-0: {want[0]} logical failures, {want[1]} rows BP left unconverged, of 3000")
        assert want[1] > 0
        for chunk in (3000, 64):
            assert eng.simulate_b8(SEED, 0, 3000, chunk=chunk, with_osd=True) == want, f"chunk {chunk}"
    finally:
        eng.close()
    got = MonteCarloDemSimulation((check, obs, pri), target_run_count=3000, batch_size=1024, seed=SEED, max_iter=12, memory_strength=g).run()
    assert (got["fail_count"], got["bp_unconverged_count"]) == want


# ---- 5. the C ABI: refusals, buffers ------------------------------------------------------------------------------------------------------------
def test_cabi_refusals():
    from ldpc_amd import _lib
    c, g = _small("hamming3", 0.625)
    n = c["h"].shape[1]
    eng = _engine(c, g)
    lib = eng._lib
    try:
        # the setter: -1 (LDPC_HIP_ERR_INVALID), and the strengths it held stay
        for bad in (1.0, -1.5, float("nan"), float("inf")):
            v = np.full(n, 0.1)
            v[3] = bad
            assert lib.ldpc_hip_bp_set_memory(eng._h, v.ctypes.data_as(C.c_void_p)) == -1
            assert b"memory strength 3" in lib.ldpc_hip_last_error() and b"[-1, 1)" in lib.ldpc_hip_last_error()
            with pytest.raises(ValueError, match=r"memory strength 3"):
                eng.set_memory(v)
        assert np.array_equal(eng.memory(), g)
        assert lib.ldpc_hip_bp_set_memory(None, None) == -1 and lib.ldpc_hip_bp_get_memory(None, None) == -1
        # the modes, each with its message, nothing launched
        probs_rows = np.tile(np.clip(c["probs"], 0.01, 0.99), (len(c["synd"]), 1))
        with launch_util.launch_log() as log:
            eng.set_params(c["max_iter"], 0, 1.0)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: memory min-sum: product-sum"):
                eng.decode_batch(c["synd"])
            eng.set_params(c["max_iter"], 1, 0.625)
            for schedule in ("serial", "serial_relative"):
                eng.set_schedule(schedule)
                with pytest.raises(_lib.LdpcHipError, match=r"error -4: memory min-sum: the serial schedules"):
                    eng.decode_batch(c["synd"])
            eng.set_schedule("parallel")
            eng.set_random_serial(True, 5)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: memory min-sum: the serial schedules"):
                eng.decode_batch(c["synd"])
            eng.set_random_serial(False, 5)
            eng.set_message_dtype("float32")
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: memory min-sum: float32 messages"):
                eng.decode_batch(c["synd"])
            eng.set_message_dtype("float64")
            for osd0 in (False, True):
                with pytest.raises(_lib.LdpcHipError, match=r"error -4: memory min-sum: per-row channel probabilities"):
                    eng.decode_batch(c["synd"], osd0=osd0, channel_probs=probs_rows)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: memory min-sum: soft-syndrome"):
                eng.soft_info_decode_batch(np.ones((2, 3)), np.inf, 2.0)
            # a nonzero strength on the p = 0 column: refused at decode time, naming what it needs
            v = g.copy()
            assert c["probs"][0] == 0.0 and v[0] == 0.0
            v[0] = 0.2
            eng.set_memory(v)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: memory min-sum: column 0 .*strictly between 0 and 1"):
                eng.decode_batch(c["synd"])
            eng.set_osd(1, 0)
            with pytest.raises(_lib.LdpcHipError, match=r"strictly between 0 and 1"):
                eng.decode_batch(c["synd"], osd=True)
        assert not [k for k in log if k.startswith("bp_")], f"a refusal launched a BP kernel: {sorted(log)}"
        assert not log, f"a refused decode launched something: {sorted(log)}"
        # ... and the handle still decodes
        eng.set_memory(g)
        _same(eng.decode_batch(c["synd"]), _checked("hamming3_a0.625|mixed", c, g), "after the refusals")
    finally:
        eng.close()


def test_close_frees_every_device_buffer():
    from ldpc_amd import _lib
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    for c, mode in ((mu.first_rows(mu.edge_case("bb144"), 70), None), (mu.first_rows(mu.edge_case("bb144"), 70), 0), (fu.irregular_case(), None)):
        eng = _engine(c, np.full(c["h"].shape[1], 0.35), mode=mode)
        try:
            eng.decode_batch(c["synd"])
            eng.set_memory(None)
            eng.decode_batch(c["synd"])
            eng.set_memory(np.full(c["h"].shape[1], -0.2))
            eng.set_osd(1, 0)
            eng.decode_batch(c["synd"], osd=True)
            during = held()
        finally:
            eng.close()
        after = held()
        print(f"memory min-sum: device buffer bytes before {before}, with the engine {during}, after close {after}")
        assert during > before and after == before, f"{after - before} bytes of device buffers outlive the handle"
