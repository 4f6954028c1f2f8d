"""The detector-error-model sampler on the host: thresholds, the NumPy twin (the specification the device reproduces), validation, the
C symbols, and the host arithmetic of the library under the host sanitizers (a stand-alone program: nothing loaded into Python, no GPU)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from window_util import phenomenological_dem, phenomenological_matrices, ring_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dem_models():
    """The three models of the sampler tests: name -> (check, observables, priors)."""
    from ldpc_amd.codes import hamming_code
    from ldpc_amd.codes.synthetic import bivariate_bicycle_hx
    out = {}
    for name, h, rounds in (("ring8x6", ring_code(8), 6), ("hamming3x7", hamming_code(3), 7), ("bb144x3", bivariate_bicycle_hx(), 3)):
        p_data = [0.01 + 0.01 * (j % 5) for j in range(h.shape[1])]
        out[name] = phenomenological_matrices(h, rounds, p_data, 0.02)
    return out


def unpack(b8, bits):
    return np.unpackbits(b8, axis=1, bitorder="little", count=bits) if bits else np.zeros((b8.shape[0], 0), np.uint8)


def test_thresholds_array_form_equals_the_scalar_one():
    from ldpc_amd.prng import bernoulli_threshold, bernoulli_thresholds
    ps = [0, 1, 0.5, 1e-300, 1 - 2.0 ** -53, 0.001, 0.09, 2.0 ** -53, 2.0 ** -54]
    got = bernoulli_thresholds(ps)
    assert got.dtype == np.uint64 and got.shape == (9,)
    assert [int(t) for t in got] == [bernoulli_threshold(float(p)) for p in ps]
    assert [int(t) for t in got[[0, 1, 2, 3, 4, 7, 8]]] == [0, 2 ** 53, 2 ** 52, 1, 2 ** 53 - 1, 1, 1]
    assert bernoulli_thresholds(np.full((2, 3), 0.25)).shape == (2, 3)
    for bad in ([0.1, -0.1], [1.5], [float("nan")]):
        with pytest.raises(ValueError):
            bernoulli_thresholds(bad)


def test_twin_with_uniform_probabilities_is_the_bsc_generator():
    from ldpc_amd.noise_models import generate_bsc_batch, generate_dem_batch
    check, obs, _ = dem_models()["ring8x6"]
    assert check.shape[1] == 88
    errors, dets, true_obs = generate_dem_batch(check, obs, np.full(88, 0.03), 5, 1000, 70)
    e = generate_bsc_batch(88, 0.03, seed=5, shot0=1000, shots=70)
    assert np.array_equal(unpack(errors, 88), e)
    assert np.array_equal(unpack(dets, 48), (sp.csr_matrix(check) @ e.T % 2).T)
    assert np.array_equal(unpack(true_obs, 1), (sp.csr_matrix(obs) @ e.T % 2).T)
    assert dets.shape == (70, 6) and true_obs.shape == (70, 1) and errors.shape == (70, 11)


def test_twin_shards_and_large_shot_index():
    from ldpc_amd.noise_models import generate_dem_batch
    check, obs, pri = dem_models()["hamming3x7"]
    whole = generate_dem_batch(check, obs, pri, 3, 0, 100)
    a, b = generate_dem_batch(check, obs, pri, 3, 0, 37), generate_dem_batch(check, obs, pri, 3, 37, 63)
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(w, np.concatenate([x, y]))
    far = generate_dem_batch(check, obs, pri, 3, 2 ** 40, 5)  # (2**40 * 67 passes 2**32: the index is taken in uint64)
    from ldpc_amd.prng import bernoulli_thresholds, sm64_int
    thr = bernoulli_thresholds(pri)
    n = check.shape[1]
    want = [[int((sm64_int(3, ((2 ** 40 + b) * n + j) % 2 ** 64) >> 11) < int(thr[j])) for j in range(n)] for b in range(5)]
    assert np.array_equal(unpack(far[0], n), np.array(want, np.uint8))
    # padding bits are zero
    assert not (far[0][:, -1] >> (n % 8)).any() and not (far[1][:, -1] >> (check.shape[0] % 8)).any() and not (far[2][:, -1] >> 1).any()


@pytest.mark.parametrize("name", ["ring8x6", "hamming3x7", "bb144x3"])
def test_twin_column_frequencies(name):
    """Every column fires with its own probability: 4096 shots, each frequency within 5 standard deviations of a binomial's mean
    (the largest deviation on these three models is 3.67)."""
    from ldpc_amd.noise_models import generate_dem_batch
    check, obs, pri = dem_models()[name]
    shots = 4096
    errors, _, _ = generate_dem_batch(check, obs, pri, 11, 0, shots)
    freq = unpack(errors, check.shape[1]).mean(axis=0)
    z = np.abs(freq - pri) / np.sqrt(pri * (1 - pri) / shots)
    print(f"{name}: largest deviation {z.max():.2f} standard deviations")
    assert z.max() <= 5.0


def test_twin_probabilities_zero_and_one():
    from ldpc_amd.noise_models import generate_dem_batch
    check, obs, pri = dem_models()["ring8x6"]
    pri = pri.copy()
    pri[3], pri[40] = 0.0, 1.0
    e = unpack(generate_dem_batch(check, obs, pri, 1, 0, 500)[0], 88)
    assert not e[:, 3].any() and e[:, 40].all()


def test_validation():
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from ldpc_amd.noise_models import generate_dem_batch
    check, obs, pri = dem_models()["ring8x6"]
    for bad in (np.where(np.arange(88) == 5, 1.5, pri), np.where(np.arange(88) == 5, -0.1, pri), np.where(np.arange(88) == 5, np.nan, pri), pri[:-1]):
        with pytest.raises(ValueError):
            generate_dem_batch(check, obs, bad, 0, 0, 4)
        with pytest.raises(ValueError):
            MonteCarloDemSimulation((check, obs, bad), target_run_count=10)
    model = (check, obs, pri)
    for kwargs in (dict(target_run_count=0), dict(target_run_count=2.5), dict(target_run_count=10, batch_size=0),
                   dict(target_run_count=10, seed=-1), dict(target_run_count=10, seed="a"), dict(target_run_count=10, message_dtype="float16"),
                   dict(target_run_count=10, osd_method="nope"), dict(target_run_count=10, bp_method="nope"),
                   dict(target_run_count=10, window_decoder=object()), dict(target_run_count=10, max_iter=-1)):
        with pytest.raises(ValueError):
            MonteCarloDemSimulation(model, **kwargs)
    with pytest.raises(ValueError):
        MonteCarloDemSimulation(None, target_run_count=10)
    with pytest.raises(ValueError):
        MonteCarloDemSimulation((check, obs[:, :-1], pri), target_run_count=10)
    with pytest.raises(TypeError):
        MonteCarloDemSimulation(model)  # target_run_count is required


def test_models_from_text_and_matrices_agree():
    """DEM text, its DemMatrices and the matrices built directly describe one model: same shapes, priors and sample."""
    from ldpc_amd.ckt_noise.dem_matrices import detector_error_model_to_check_matrices
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    p_data = [0.01 + 0.01 * (j % 5) for j in range(8)]
    text = phenomenological_dem(ring_code(8), 6, p_data, 0.02)
    sims = [MonteCarloDemSimulation(text, target_run_count=10),
            MonteCarloDemSimulation(detector_error_model_to_check_matrices(text, allow_undecomposed_hyperedges=True), target_run_count=10),
            MonteCarloDemSimulation(phenomenological_matrices(ring_code(8), 6, p_data, 0.02), target_run_count=10)]
    for s in sims[1:]:
        assert (s.check_matrix != sims[0].check_matrix).nnz == 0 and (s.observables_matrix != sims[0].observables_matrix).nnz == 0
        assert np.allclose(s.priors, sims[0].priors, rtol=0, atol=1e-15)
    assert sims[0].save() == {"logical_error_rate": 0.0, "logical_error_rate_eb": 0.0, "error_rate": sims[0].error_rate, "run_count": 0,
                              "fail_count": 0, "bp_unconverged_count": 0, "seed": 0}


def test_new_c_symbols_refuse_a_null_handle():
    from ldpc_amd import _lib
    lib = _lib.load()
    for name in ("ldpc_hip_bp_set_sampler", "ldpc_hip_bp_sample_b8", "ldpc_hip_count_mismatch_b8", "ldpc_hip_bp_simulate_b8"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    out = (ctypes.c_uint64 * 2)()
    assert lib.ldpc_hip_bp_set_sampler(None, None) == -1
    assert b"null" in lib.ldpc_hip_last_error()
    assert lib.ldpc_hip_bp_sample_b8(None, 1, 0, 4, None, None, None) == -1
    assert lib.ldpc_hip_count_mismatch_b8(None, None, None, 4, 8, out, None) == -1
    assert lib.ldpc_hip_bp_simulate_b8(None, 1, 0, 4, 0, 0, out) == -1


def test_host_arithmetic_under_the_host_sanitizers(tmp_path):
    """ldpc_amd/csrc/dem_host.h (probabilities -> thresholds, rows -> columns of L) in tools/dem_host_check.cpp, built with
    -fsanitize=address,undefined and run on its own."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (build() uses one too)"
    exe = str(tmp_path / "dem_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", os.path.join(ROOT, "ldpc_amd", "csrc"), os.path.join(ROOT, "tools", "dem_host_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "dem_host_check ok" in run.stdout, run.stdout + run.stderr
