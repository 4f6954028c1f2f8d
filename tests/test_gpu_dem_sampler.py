"""The detector-error-model sampler, the mismatch count and the sample -> decode -> compare loop on the device, against the NumPy twin
(noise_models.generate_dem_batch: the specification) and against the host loop twin -> decode_b8 -> compare."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import launch_util as lu
from test_dem_sampler_twin import dem_models, unpack
from window_util import phenomenological_dem, phenomenological_matrices, ring_code

pytestmark = pytest.mark.gpu

MODELS = ("ring8x6", "hamming3x7", "bb144x3")  # n = 88, 67, 576 (two and nine lane steps, a ragged last one); m = 48, 21, 216 (rows of 6, 3, 27 bytes)
SEED = 7


@functools.lru_cache(maxsize=None)
def model(name, wide_l=False):
    """(check csr, observables csr, priors): the model's own single observable row, or with nine random rows beside it (two bytes)."""
    check, obs, pri = dem_models()[name]
    obs = sp.csr_matrix(obs, dtype=np.uint8)
    if wide_l:
        rng = np.random.default_rng(len(name))
        obs = sp.csr_matrix((rng.random((9, check.shape[1])) < 0.2).astype(np.uint8))
    return sp.csr_matrix(check, dtype=np.uint8), obs, pri


@functools.lru_cache(maxsize=None)
def twin(name, wide_l, shot0, shots=3000):
    from ldpc_amd.noise_models import generate_dem_batch
    check, obs, pri = model(name, wide_l)
    out = generate_dem_batch(check, obs, pri, SEED, shot0, shots)
    for a in out:
        a.setflags(write=False)
    return out


def engine(check, pri, obs=None, sampler="own", max_iter=12, **switches):
    from ldpc_amd.engine import HipBpEngine
    h = sp.csr_matrix(check, dtype=np.uint8)
    h.sort_indices()
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], np.clip(pri, 1e-9, 1 - 1e-9), max_iter, 1, 0.625)
    if obs is not None:
        eng.set_observables(obs)
    if sampler == "own":
        eng.set_sampler(pri)
    for name, value in switches.items():
        eng.set_debug_switch(name, value)
    return eng


def to_numpy(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


@pytest.mark.parametrize("place", ["host", "device"])
@pytest.mark.parametrize("wide_l", [False, True], ids=["k1", "k9"])
@pytest.mark.parametrize("name", MODELS)
def test_sample_equals_the_twin(name, wide_l, place):
    import torch
    check, obs, pri = model(name, wide_l)
    eng = engine(check, pri, obs)
    device = torch.device("cuda", torch.cuda.current_device()) if place == "device" else None
    with lu.launch_log() as log:
        for shot0 in (0, 2 ** 40):
            want = twin(name, wide_l, shot0)
            for batch in (1, 70, 3000):
                dets, true_obs, errors = eng.sample_b8(SEED, shot0, batch, device=device, want_errors=True)
                for got, ref, what in ((errors, want[0], "errors"), (dets, want[1], "detection events"), (true_obs, want[2], "observables")):
                    got = to_numpy(got)
                    assert got.shape == (batch, ref.shape[1]) and got.dtype == np.uint8
                    assert np.array_equal(got, ref[:batch]), f"{what} differ from the twin (shot0 {shot0}, batch {batch})"
    lu.assert_ran(log, "dem_sample_b8_kernel")
    assert log["dem_sample_b8_kernel"] == 6


def test_sample_without_errors_or_observables():
    check, obs, pri = model("hamming3x7")
    want = twin("hamming3x7", False, 0)
    eng = engine(check, pri)  # no observables set
    dets, none = eng.sample_b8(SEED, 0, 70)
    assert none is None and np.array_equal(dets, want[1][:70])
    eng.set_observables(obs)  # ... after the sampler: the column view of L is built by whichever comes second
    dets, true_obs = eng.sample_b8(SEED, 0, 70)
    assert np.array_equal(dets, want[1][:70]) and np.array_equal(true_obs, want[2][:70])
    assert eng.sample_b8(SEED, 5, 0)[0].shape == (0, 3)  # batch 0 is fine


def test_edge_cases_in_the_matrices():
    """Probabilities 0 and 1, an L with an empty row, a column of H with no entry, k = 0."""
    from ldpc_amd.noise_models import generate_dem_batch
    check, _, pri = model("ring8x6", True)
    check = check.tolil()
    check[:, 17] = 0
    check = sp.csr_matrix(check)
    check.eliminate_zeros()
    pri = pri.copy()
    pri[3], pri[40], pri[17] = 0.0, 1.0, 1.0
    rng = np.random.default_rng(3)
    obs = (rng.random((9, 88)) < 0.2).astype(np.uint8)
    obs[4] = 0
    for obs_m in (sp.csr_matrix(obs), sp.csr_matrix((0, 88), dtype=np.uint8)):
        want = generate_dem_batch(check, obs_m, pri, SEED, 11, 500)
        eng = engine(check, pri, obs_m)
        dets, true_obs, errors = eng.sample_b8(SEED, 11, 500, want_errors=True)
        assert np.array_equal(errors, want[0]) and np.array_equal(dets, want[1]) and np.array_equal(true_obs, want[2])
        e = unpack(errors, 88)
        assert not e[:, 3].any() and e[:, 40].all() and e[:, 17].all()
        assert true_obs.shape == (500, (obs_m.shape[0] + 7) // 8)


@pytest.mark.parametrize("grid", [1, 3])
def test_capped_grid_loops_over_the_shots(grid):
    import torch
    check, obs, pri = model("bb144x3", True)
    want = twin("bb144x3", True, 0)
    eng = engine(check, pri, obs, DEM_GRID=grid)
    dets, true_obs, errors = eng.sample_b8(SEED, 0, 3000, device=torch.device("cuda", torch.cuda.current_device()), want_errors=True)
    assert np.array_equal(to_numpy(errors), want[0]) and np.array_equal(to_numpy(dets), want[1]) and np.array_equal(to_numpy(true_obs), want[2])


def test_uniform_probabilities_are_the_bsc_generator_and_shards_are_the_whole():
    check, obs, _ = model("ring8x6")
    eng = engine(check, np.full(88, 0.03), obs)
    synd, err = eng.gen_bsc_syndromes(5, 0.03, 1000, 70, want_errors=True)
    dets, _, errors = eng.sample_b8(5, 1000, 70, want_errors=True)
    assert np.array_equal(unpack(errors, 88), err) and np.array_equal(unpack(dets, 48), synd)
    whole = eng.sample_b8(5, 0, 100, want_errors=True)
    a, b = eng.sample_b8(5, 0, 37, want_errors=True), eng.sample_b8(5, 37, 63, want_errors=True)
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(w, np.concatenate([x, y]))


def test_sampler_follows_set_sampler_not_the_decoding_priors():
    check, obs, pri = model("hamming3x7")
    want = twin("hamming3x7", False, 0)
    eng = engine(check, pri, obs, sampler=None)
    eng.set_sampler()  # None: the handle's channel probabilities
    assert np.array_equal(eng.sample_b8(SEED, 0, 70)[0], want[1][:70])
    eng.set_channel(np.full(67, 0.2))  # decoding priors change; the sampler does not
    assert np.array_equal(eng.sample_b8(SEED, 0, 70)[0], want[1][:70])
    with pytest.raises(ValueError):
        eng.set_sampler(np.full(66, 0.1))
    with pytest.raises(ValueError):
        eng.set_sampler(np.where(np.arange(67) == 2, np.nan, 0.1))
    bad = np.full(67, 1.5)
    assert eng._lib.ldpc_hip_bp_set_sampler(eng._h, bad.ctypes.data) == -1  # the library checks for itself


def test_refusals():
    from ldpc_amd._lib import LdpcHipError
    check, obs, pri = model("hamming3x7")
    eng = engine(check, pri, sampler=None)
    with pytest.raises(LdpcHipError, match="-1.*set_sampler"):
        eng.sample_b8(SEED, 0, 4)
    eng.set_sampler(pri)
    dets, obs_out = np.zeros((4, 3), np.uint8), np.zeros((4, 1), np.uint8)
    lib = eng._lib
    assert lib.ldpc_hip_bp_sample_b8(eng._h, SEED, 0, 4, dets.ctypes.data, obs_out.ctypes.data, None) == -1  # obs_b8 without observables
    assert b"set_observables" in lib.ldpc_hip_last_error()
    out = (ctypes.c_uint64 * 2)()
    assert lib.ldpc_hip_bp_simulate_b8(eng._h, SEED, 0, 4, 0, 0, out) == -1
    eng.set_observables(obs)
    assert lib.ldpc_hip_bp_sample_b8(eng._h, SEED, -1, 4, dets.ctypes.data, None, None) == -1
    assert lib.ldpc_hip_bp_sample_b8(eng._h, SEED, 0, -4, dets.ctypes.data, None, None) == -1
    assert lib.ldpc_hip_bp_sample_b8(eng._h, SEED, 0, 0, None, None, None) == 0
    assert lib.ldpc_hip_bp_simulate_b8(eng._h, SEED, 0, -4, 0, 0, out) == -1


def test_detectors_beyond_the_lds_bound_are_refused_before_any_launch():
    """A wavefront's strips hold ceil(m / 32) + ceil(k / 32) <= 4096 words: an H with 4096 * 32 + 1 rows, most of them empty."""
    from ldpc_amd._lib import LdpcHipError
    m = 4096 * 32 + 1
    check = sp.csr_matrix((np.ones(4, np.uint8), ([0, 1, 5, m - 1], [0, 1, 2, 3])), shape=(m, 4))
    eng = engine(check, np.full(4, 0.1))
    with lu.launch_log() as log:
        with pytest.raises(LdpcHipError, match="error -4.*4096"):
            eng.sample_b8(SEED, 0, 8)
    assert not log, f"refused, yet launched: {log}"
    # one row fewer fits, with no room left for an observable
    check = sp.csr_matrix((np.ones(4, np.uint8), ([0, 1, 5, m - 2], [0, 1, 2, 3])), shape=(m - 1, 4))
    eng = engine(check, np.full(4, 0.5))
    dets, _, errors = eng.sample_b8(SEED, 0, 8, want_errors=True)
    e = unpack(errors, 4)
    assert np.array_equal(unpack(dets, m - 1)[:, [0, 1, 5, m - 2]], e) and int(unpack(dets, m - 1).sum()) == int(e.sum())
    eng.set_observables(sp.csr_matrix(np.ones((1, 4), np.uint8)))
    with pytest.raises(LdpcHipError, match="error -4"):
        eng.sample_b8(SEED, 0, 8)


@pytest.mark.parametrize("bits", [1, 8, 9, 64])
def test_count_mismatch_b8(bits):
    import torch
    check, _, pri = model("hamming3x7")
    eng = engine(check, pri)
    rng = np.random.default_rng(bits)
    nb = (bits + 7) // 8
    rows = 1000
    a = rng.integers(0, 256, (rows, nb), dtype=np.uint8)
    b = a.copy()
    flip = rng.random(rows) < 0.3
    which = rng.integers(0, bits, rows)
    b[flip, which[flip] // 8] ^= (1 << (which[flip] % 8)).astype(np.uint8)
    want = int(np.count_nonzero((unpack(a, bits) != unpack(b, bits)).any(axis=1)))
    assert want == int(flip.sum()) and want > 0
    assert eng.count_mismatch_b8(a, b, bits) == want
    dev = torch.device("cuda", torch.cuda.current_device())
    assert eng.count_mismatch_b8(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), bits) == want
    if bits % 8:  # padding bits set in one operand only do not count
        b2 = b.copy()
        b2[:, -1] |= np.uint8((0xFF << (bits % 8)) & 0xFF)
        assert eng.count_mismatch_b8(a, b2, bits) == want
    # per-row flags through the C ABI
    flags, count = np.full(rows, 7, np.uint8), ctypes.c_uint64(99)
    assert eng._lib.ldpc_hip_count_mismatch_b8(eng._h, a.ctypes.data, b.ctypes.data, rows, bits, ctypes.addressof(count), flags.ctypes.data) == 0
    assert count.value == want and np.array_equal(flags.astype(bool), flip)
    assert eng.count_mismatch_b8(a[:0], b[:0], bits) == 0


SIMULATE_CASES = {
    "ring8x6": dict(name="ring8x6"),
    "hamming3x7": dict(name="hamming3x7"),
    "bb144x3": dict(name="bb144x3"),
    "bb144x3-osd0": dict(name="bb144x3", osd=(1, 0)),
    "bb144x3-osdcs4": dict(name="bb144x3", osd=(3, 4)),
    "ring8x6-f32": dict(name="ring8x6", dtype="float32"),
}


@pytest.mark.parametrize("case", list(SIMULATE_CASES))
def test_simulate_b8_equals_the_host_loop(case):
    """Min-sum 12 (+ OSD where named) over 3000 shots: both counters equal twin -> decode_b8 from NumPy -> compare, whatever the chunk."""
    cfg = SIMULATE_CASES[case]
    check, obs, pri = model(cfg["name"])
    eng = engine(check, pri, obs)
    with_osd = "osd" in cfg
    if with_osd:
        eng.set_osd(*cfg["osd"])
    eng.set_message_dtype(cfg.get("dtype", "float64"))
    _, dets, true_obs = twin(cfg["name"], False, 0)
    pred, _, _, conv = eng.decode_b8(np.array(dets), with_osd=with_osd)
    want = (int(np.count_nonzero((pred != true_obs).any(axis=1))), int(np.count_nonzero(~conv)))
    print(f"{case}: {want[0]} logical failures, {want[1]} rows BP left unconverged, of 3000")
    assert want[0] > 0 or want[1] > 0, "the case should have something to count"
    with lu.launch_log() as log:
        for chunk in (3000, 1000, 64, 0):
            assert eng.simulate_b8(SEED, 0, 3000, chunk=chunk, with_osd=with_osd) == want, f"chunk {chunk}"
    lu.assert_ran(log, "dem_sample_b8_kernel", "mismatch_b8_kernel")
    # disjoint shot ranges add up
    a, b = eng.simulate_b8(SEED, 0, 1234, with_osd=with_osd), eng.simulate_b8(SEED, 1234, 1766, with_osd=with_osd)
    assert (a[0] + b[0], a[1] + b[1]) == want
    assert eng.simulate_b8(SEED, 0, 0) == (0, 0)


def test_simulate_b8_keeps_the_float32_refusals():
    from ldpc_amd._lib import LdpcHipError
    check, obs, pri = model("ring8x6")
    eng = engine(check, pri, obs)
    eng.set_params(12, 0, 1.0)  # product-sum
    eng.set_message_dtype("float32")
    with pytest.raises(LdpcHipError, match="-4"):
        eng.simulate_b8(SEED, 0, 100)
    with pytest.raises(LdpcHipError, match="-4"):
        eng.decode_b8(np.zeros((4, 6), np.uint8))


def _p_data(n):
    return [0.01 + 0.01 * (j % 5) for j in range(n)]


def test_monte_carlo_from_text_and_from_matrices_and_in_two_runs():
    from ldpc_amd.codes import hamming_code
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    kw = dict(batch_size=700, seed=SEED, max_iter=12)
    text = phenomenological_dem(hamming_code(3), 7, _p_data(7), 0.02)
    mats = phenomenological_matrices(hamming_code(3), 7, _p_data(7), 0.02)
    one = MonteCarloDemSimulation(text, target_run_count=3000, **kw).run()
    assert one == MonteCarloDemSimulation(mats, target_run_count=3000, **kw).run()
    assert one["run_count"] == 3000 and one["seed"] == SEED
    assert one["logical_error_rate"] == one["fail_count"] / 3000
    # the host loop over the same sample
    check, obs, pri = model("hamming3x7")
    eng = engine(check, pri, obs)
    eng.set_osd(1, 0)
    _, dets, true_obs = twin("hamming3x7", False, 0)
    pred, _, _, conv = eng.decode_b8(np.array(dets), with_osd=True)
    want = (int(np.count_nonzero((pred != true_obs).any(axis=1))), int(np.count_nonzero(~conv)))
    print(f"hamming3x7, min-sum 12 + OSD-0: {want[0]} logical failures, {want[1]} rows BP left unconverged, of 3000")
    assert (one["fail_count"], one["bp_unconverged_count"]) == want
    # to 1000, then on to 3000: the totals of one long run
    sim = MonteCarloDemSimulation(text, target_run_count=1000, **kw)
    first = sim.run()
    assert first["run_count"] == 1000 and first["fail_count"] <= one["fail_count"]
    sim.target_run_count = 3000
    assert sim.run() == one


def test_monte_carlo_with_a_window_decoder():
    """ring8 x 6 rounds at a noise level where the windows do fail now and then, 2 windows of 4 rounds committing 2: the simulation's count
    equals the twin's shots put through the decoder's own decode_batch and compared on the host."""
    from ldpc_amd.ckt_noise import BpOsdOverlappingWindowDecoder
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from ldpc_amd.noise_models import generate_dem_batch
    p_data = [0.08 + 0.01 * (j % 5) for j in range(8)]
    text = phenomenological_dem(ring_code(8), 6, p_data, 0.08)
    mats = phenomenological_matrices(ring_code(8), 6, p_data, 0.08)
    cfg = dict(max_iter=6, bp_method="minimum_sum", ms_scaling_factor=0.8, osd_method="osd0", osd_order=0)

    def decoder():
        return BpOsdOverlappingWindowDecoder(text, decodings=2, window=4, commit=2, num_checks=8, decoder_config=cfg)

    got = MonteCarloDemSimulation(text, target_run_count=3000, batch_size=1100, seed=SEED, window_decoder=decoder()).run()
    _, dets, true_obs = generate_dem_batch(*mats, SEED, 0, 3000)
    pred = decoder().decode_batch(unpack(dets, 48))
    want = int(np.count_nonzero((pred != unpack(true_obs, 1).astype(bool)).any(axis=1)))
    print(f"window decoder: {want} logical failures of 3000")
    assert want > 0, "the windows should fail now and then at this noise level (177 of 3000 when this was written)"
    assert got["fail_count"] == want and got["run_count"] == 3000 and got["bp_unconverged_count"] is None


def _host_loop(check, obs, sample_priors, decode_priors, shots=3000, dtype="float64"):
    """(failures, unconverged) of twin -> decode_b8 from NumPy (min-sum 12 + OSD-0) -> compare."""
    from ldpc_amd.noise_models import generate_dem_batch
    eng = engine(check, decode_priors, obs, sampler=None)
    eng.set_osd(1, 0)
    eng.set_message_dtype(dtype)
    _, dets, true_obs = generate_dem_batch(check, obs, sample_priors, SEED, 0, shots)
    pred, _, _, conv = eng.decode_b8(dets, with_osd=True)
    return int(np.count_nonzero((pred != true_obs).any(axis=1))), int(np.count_nonzero(~conv))


def test_monte_carlo_with_float32_messages():
    """message_dtype='float32' through the class: min-sum + OSD-0 is not among the float32 refusals; product-sum is, at run()."""
    from ldpc_amd._lib import LdpcHipError
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    check, obs, pri = model("bb144x3")
    want = _host_loop(check, obs, pri, pri, dtype="float32")
    got = MonteCarloDemSimulation((check, obs, pri), target_run_count=3000, batch_size=1024, seed=SEED, max_iter=12, message_dtype="float32").run()
    print(f"bb144x3 float32, min-sum 12 + OSD-0: {want[0]} logical failures, {want[1]} rows BP left unconverged, of 3000")
    assert want[0] > 0 or want[1] > 0
    assert (got["fail_count"], got["bp_unconverged_count"]) == want
    with pytest.raises(LdpcHipError, match="-4"):
        MonteCarloDemSimulation((check, obs, pri), target_run_count=100, seed=SEED, bp_method="ps", message_dtype="float32").run()


def test_monte_carlo_with_mechanisms_at_probability_zero_and_one():
    """A model with p = 0 and p = 1 among its mechanisms: sampled exactly (never / always), decoded with the priors clipped to
    [1e-9, 1 - 1e-9] -- the counts are those of the host loop that samples with the model's values and decodes with the clipped ones."""
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from ldpc_amd.monte_carlo_simulation.dem_mcs import DECODING_PRIOR_FLOOR
    check, obs, pri = model("hamming3x7")
    pri = pri.copy()
    pri[5], pri[30], pri[31] = 0.0, 1.0, 0.0
    assert DECODING_PRIOR_FLOOR == 1e-9  # (what engine() clips to)
    want = _host_loop(check, obs, pri, pri)
    got = MonteCarloDemSimulation((check, obs, pri), target_run_count=3000, batch_size=2000, seed=SEED, max_iter=12).run()
    print(f"hamming3x7 with p = 0 / 1 columns: {want[0]} logical failures, {want[1]} rows BP left unconverged, of 3000")
    assert want[0] > 0 or want[1] > 0
    assert (got["fail_count"], got["bp_unconverged_count"]) == want
