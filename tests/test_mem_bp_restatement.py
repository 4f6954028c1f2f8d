"""Memory min-sum BP without a GPU: the NumPy restatement (tests/mem_bp_util.py) against the plain one at strength 0, the library's host
arithmetic for a[] (ldpc_amd/csrc/mem_host.h) as a stand-alone program under the host sanitizers, the setter's validation, and what the
Python decoders refuse -- each before any handle exists."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import f32_util as fu
import mem_bp_util as mu
from oracle import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["hamming3", "rep5", "irregular"])
def test_strength_zero_is_the_plain_restatement(key):
    c = {"hamming3": lambda: fu.small_case("hamming3", 0.625), "rep5": lambda: fu.small_case("rep5", 0.0), "irregular": fu.irregular_case}[key]()
    want = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], c["max_iter"], c["alpha"], np.float64)
    got = mu.min_sum_memory_restatement(c["h"], c["probs"], np.zeros(c["h"].shape[1]), c["synd"], c["max_iter"], c["alpha"])
    for k, name in ((0, "decoding"), (2, "iterations"), (3, "converge")):
        assert np.array_equal(got[k], want[k]), f"{key}: {name}"
    assert bits_equal(got[1], want[1]), f"{key}: log-ratios differ in some bit"
    assert want[3].any() and not want[3].all()


def test_a_nonzero_strength_changes_something_and_zero_columns_keep_infinite_priors():
    c = fu.small_case("hamming3", 0.625)
    g = mu.mixed_gamma(c["probs"])
    assert (g[(c["probs"] == 0.0) | (c["probs"] == 1.0)] == 0.0).all() and (g[c["probs"] == 0.5] != 0.0).all()
    assert (g < 0).any() and (g > 0).any() and (g == 0).any()
    want = mu.min_sum_memory_restatement(c["h"], c["probs"], g, c["synd"], c["max_iter"], c["alpha"])
    mu.assert_shows_something(want, mu.plain("hamming3_a0.625", c), c["max_iter"], "hamming3")
    a = mu.memory_a(c["probs"], g)
    assert a[0] == np.inf and a[1] == -np.inf and not np.signbit(a[c["probs"] == 0.5]).any()


@pytest.mark.parametrize("code", ["surface5", "bb144", "hgp_hamming3"])
def test_edge_cases_show_something(code):
    """The noise and max_iter of the lane = edge cases were picked so that their first 70 rows already converge here and not there, and
    differ from the plain decode -- with the scalar strength and with the drawn one (the GPU tests assert it again on what they compare)."""
    c = mu.first_rows(mu.edge_case(code), 70)
    n = c["h"].shape[1]
    for tag, g in (("scalar", np.full(n, 0.35)), ("drawn", mu.drawn_gamma(n, 7))):
        want = mu.min_sum_memory_restatement(c["h"], c["probs"], g, c["synd"], c["max_iter"], c["alpha"])
        plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], c["max_iter"], c["alpha"], np.float64)
        mu.assert_shows_something(want, plain, c["max_iter"], f"{code}/{tag}")


# ---- a[] as the library's host code forms it ------------------------------------------------------------------------------------------------
def test_host_arithmetic_under_the_host_sanitizers(tmp_path):
    """ldpc_amd/csrc/mem_host.h in tools/mem_host_check.cpp, built with -fsanitize=address,undefined and run on its own: its own checks, and
    a[] of the shared cases' channels and strengths against the restatement's, bit for bit."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (build() uses one too)"
    exe = str(tmp_path / "mem_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "ldpc_amd", "csrc"),
                    os.path.join(ROOT, "tools", "mem_host_check.cpp"), "-o", exe], check=True)
    probs = np.concatenate([fu._edge_channel(24), [0.03, 0.06, 1e-9, 1 - 1e-9, 0.5]])
    gamma = np.concatenate([mu.mixed_gamma(fu._edge_channel(24)), [0.35, -1.0, 1 - 2.0 ** -53, 0.66, -0.24]])
    args = [x for p, g in zip(probs, gamma) for x in (float(p).hex(), float(g).hex())]
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == 0 and "mem_host_check ok" in run.stdout, run.stdout + run.stderr
    got = np.array([int(line.split()[1], 16) for line in run.stdout.splitlines() if line.startswith("a ")], np.uint64)
    want = mu.memory_a(probs, gamma)
    assert np.array_equal(got, want.view(np.uint64)), "a[] of the host code differs from the restatement's in some bit"
    assert "bad -1" in run.stdout
    assert not np.signbit(want[want == 0.0]).any(), "a[] is never -0.0"


# ---- the setter --------------------------------------------------------------------------------------------------------------------------------
def _decoder(cls=None, **kw):
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.codes import hamming_code
    args = dict(error_rate=0.05, max_iter=8, bp_method="minimum_sum", ms_scaling_factor=0.625)
    args.update(kw)
    return (cls or BpDecoder)(hamming_code(3), **args)


def test_memory_strength_property():
    d = _decoder()
    assert d.memory_strength is None
    d.memory_strength = 0.35
    got = d.memory_strength
    assert got.dtype == np.float64 and got.shape == (7,) and (got == 0.35).all()
    got[0] = 0.9
    assert d.memory_strength[0] == 0.35, "the getter hands out a copy"
    g = np.array([-0.24, 0.0, 0.35, 0.66, -1.0, 1 - 2.0 ** -53, 0.0])
    d.memory_strength = g
    assert np.array_equal(d.memory_strength, g)
    g[0] = 0.5
    assert d.memory_strength[0] == -0.24, "the setter keeps a copy"
    d.memory_strength = [0.1] * 7
    assert (d.memory_strength == 0.1).all()
    d.memory_strength = None
    assert d.memory_strength is None
    assert d._engine is None, "no handle was made"


@pytest.mark.parametrize("bad", [1.0, -1.5, float("nan"), float("inf"), -float("inf"), [0.1] * 6, [0.1] * 8, [[0.1] * 7], "x",
                                 [0.1, 0.2, 0.3, 1.0, 0.1, 0.1, 0.1], [0.1, 0.2, float("nan"), 0.3, 0.1, 0.1, 0.1]])
def test_memory_strength_validation(bad):
    d = _decoder()
    d.memory_strength = 0.25
    with pytest.raises(ValueError, match="memory_strength"):
        d.memory_strength = bad
    assert (d.memory_strength == 0.25).all(), "a refused value leaves the old one"
    assert d._engine is None


def test_memory_strength_is_no_constructor_keyword():
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    from ldpc_amd.codes import hamming_code
    with pytest.raises(ValueError, match="Unknown parameter 'memory_strength'"):
        _decoder(memory_strength=0.3)
    with pytest.raises((ValueError, TypeError), match="memory_strength"):
        BpOsdDecoder(hamming_code(3), error_rate=0.05, memory_strength=0.3)


# ---- the refusals, each before any handle exists ----------------------------------------------------------------------------------------------
def _refused(d, match, call=None):
    synd = np.array([[1, 0, 1]], np.uint8)
    with pytest.raises(NotImplementedError, match=match):
        (call or (lambda: d.decode_batch(synd)))()
    assert d._engine is None and d._cy is None, "refused before a handle was made"


def test_python_refusals():
    from ldpc_amd.bp_decoder import SoftInfoBpDecoder
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    synd = np.array([[1, 0, 1]], np.uint8)
    d = _decoder(bp_method="product_sum")
    d.memory_strength = 0.3
    _refused(d, "memory_strength with bp_method='product_sum'")
    _refused(d, "memory_strength with bp_method='product_sum'", lambda: d.decode(synd[0]))
    for schedule in ("serial", "serial_relative"):
        d = _decoder(schedule=schedule)
        d.memory_strength = 0.3
        _refused(d, f"memory_strength with schedule='{schedule}'")
    d = _decoder(random_serial_schedule=True)
    d.memory_strength = 0.3
    _refused(d, "memory_strength with schedule=.*random_serial_schedule")
    d = _decoder()
    d.memory_strength = 0.3
    d.message_dtype = "float32"
    _refused(d, "memory_strength with message_dtype='float32'")
    d = _decoder()
    d.memory_strength = 0.3
    _refused(d, "memory_strength with channel_probs", lambda: d.decode_batch(synd, channel_probs=np.full((1, 7), 0.05)))
    d = _decoder(device_ids=[0])
    d.memory_strength = 0.3
    _refused(d, r"memory_strength with device_ids=\[...\]")
    d = _decoder(cls=BpOsdDecoder, bp_method="product_sum", osd_method="osd_0")
    d.memory_strength = 0.3
    _refused(d, "memory_strength with bp_method='product_sum'")
    _refused(d, "memory_strength with bp_method='product_sum'", lambda: d.decode(synd[0]))
    s = SoftInfoBpDecoder(_decoder()._h, error_rate=0.05, max_iter=8)
    s.memory_strength = 0.3
    _refused(s, "memory_strength with soft-syndrome decoding", lambda: s.decode(np.array([1.0, -1.0, 1.0])))


def test_python_refuses_a_nonzero_strength_on_a_probability_of_0_or_1():
    d = _decoder(error_rate=None, error_channel=[0.0, 0.05, 1.0, 0.05, 0.5, 0.05, 0.05])
    d.memory_strength = [0.0, 0.3, 0.0, -0.2, 0.4, 0.0, 0.1]  # strength 0 on the p = 0 and p = 1 bits: nothing to refuse here
    d._require_modes()
    d.memory_strength = [0.0, 0.3, 0.2, -0.2, 0.4, 0.0, 0.1]
    _refused(d, "bit 2 has a nonzero memory strength.*strictly between 0 and 1")
    d.memory_strength = 0.3
    _refused(d, "bit 0 has a nonzero memory strength.*strictly between 0 and 1")


def test_dem_simulation_keyword():
    from ldpc_amd.codes import hamming_code
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from window_util import phenomenological_matrices
    model = phenomenological_matrices(hamming_code(3), 2, [0.01] * 7, 0.02)
    n = model[0].shape[1]
    sim = MonteCarloDemSimulation(model, target_run_count=10, memory_strength=0.35)
    assert sim.memory_strength.shape == (n,) and (sim.memory_strength == 0.35).all() and sim._engine is None
    assert MonteCarloDemSimulation(model, target_run_count=10).memory_strength is None
    for bad in (1.0, [0.1] * (n + 1), float("nan")):
        with pytest.raises(ValueError, match="memory_strength"):
            MonteCarloDemSimulation(model, target_run_count=10, memory_strength=bad)

    class _Window:  # (what the constructor looks at)
        num_detectors = model[0].shape[0]
        logical_observables_matrix = model[1]

        def predict_on_device(self, dets):
            raise AssertionError("never called")

    with pytest.raises(ValueError, match="memory_strength with a window_decoder"):
        MonteCarloDemSimulation(model, target_run_count=10, memory_strength=0.35, window_decoder=_Window())


def test_c_symbols_are_declared_and_listed():
    from ldpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    for name in ("ldpc_hip_bp_set_memory", "ldpc_hip_bp_get_memory"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    hpp = open(os.path.join(ROOT, "include", "ldpc_hip.hpp")).read()
    assert "bool set_memory(" in hpp and "ldpc_hip_bp_set_memory(h_" in hpp
