"""``decode_batch(..., channel_probs=P)``: a batch whose rows each carry their own channel probabilities -- everything that needs no GPU.

* the fixtures (tests/golden/row_priors/, from the reference's own ``update_channel_probs`` + ``decode`` loop) equal the CPU restatement
  row by row: ``BpOracle(error_channel=P[b])``, log-ratios compared as bit patterns (``oracle.bits_equal``);
* every refusal, with its type and what it says;
* the C ABI symbols are listed;
* the generator reproduces the committed fixtures wherever the reference is present (``--check``)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from ldpc_amd import codes
from row_priors_util import case_names, llr_digest, load_case, ran_bp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED_CASES = ["row_priors_bb144_ps10_osd0", "row_priors_hamming3_ms", "row_priors_hamming3_ps", "row_priors_irregular_n600_ms16_a0625",
                  "row_priors_irregular_n600_ms16_adaptive", "row_priors_irregular_n600_ps16", "row_priors_rep5_ms", "row_priors_rep5_ps"]


def test_every_fixture_is_there():
    assert case_names() == EXPECTED_CASES


@pytest.mark.parametrize("name", EXPECTED_CASES)
def test_fixture_equals_the_oracle_row_by_row(name):
    c = load_case(name)
    B, n = c["probs"].shape
    assert B in (70, 130) and c["syndromes"].shape == (B, c["m"])
    assert len({row.tobytes() for row in c["probs"]}) == B, "every row has its own priors"
    llr = np.zeros((B, n))
    for b in np.flatnonzero(ran_bp(c)):
        o = oracle.BpOracle(c["h"], error_channel=c["probs"][b], max_iter=c["max_iter"], bp_method=c["bp_method"],
                            ms_scaling_factor=c["ms_scaling_factor"])
        dec, l, it, cv = o.decode_batch(c["syndromes"][b:b + 1])
        llr[b] = l[0]
        assert bool(cv[0]) == bool(c["converge"][b]) and int(it[0]) == int(c["iterations"][b]), f"row {b}"
        want = dec[0] if (cv[0] or not c["osd"]) else o.osd0(c["syndromes"][b], l[0])
        assert np.array_equal(want, c["decoding"][b]), f"row {b}: decisions"
    k = len(c["llr"])
    assert oracle.bits_equal(llr[:k], c["llr"]), "log-ratios of the rows stored in full"
    assert np.array_equal(llr_digest(llr), c["llr_crc"]), "log-ratio bit patterns, every row"
    zero = ~ran_bp(c)
    assert zero.sum() == 1 and not c["decoding"][zero].any() and c["converge"][zero].all()


def _bp(**kw):
    from ldpc_amd.bp_decoder import BpDecoder
    args = dict(error_rate=0.1, max_iter=5, bp_method="product_sum", input_vector_type="syndrome")
    args.update(kw)
    return BpDecoder(codes.hamming_code(3), **args)


S = np.ones((4, 3), np.uint8)
P = np.full((4, 7), 0.1)


@pytest.mark.parametrize("bad, what", [
    (np.full((4, 6), 0.1), r"channel_probs must be a float64 array of shape \(4, 7\)"),
    (np.full((3, 7), 0.1), r"channel_probs must be a float64 array of shape \(4, 7\)"),
    (np.full(7, 0.1), r"channel_probs must be a float64 array of shape \(4, 7\)"),
    (np.full((4, 7), 0.1, np.float32), r"channel_probs must be a float64 array of shape \(4, 7\)"),
    (np.where(np.arange(28).reshape(4, 7) == 9, 1.5, 0.1), r"1 values are outside \[0, 1\] or NaN"),
    (np.where(np.eye(4, 7) > 0, -1e-9, 0.1), r"4 values are outside \[0, 1\] or NaN"),
    (np.where(np.eye(4, 7) > 0, np.nan, 0.1), r"4 values are outside \[0, 1\] or NaN"),
])
def test_value_errors(bad, what):
    with pytest.raises(ValueError, match=what):
        _bp().decode_batch(S, channel_probs=bad)


def test_syndromes_and_probabilities_in_different_places():
    import torch
    with pytest.raises(ValueError, match="same place as the syndromes"):
        _bp().decode_batch(S, channel_probs=torch.full((4, 7), 0.1, dtype=torch.float64))
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    d = BpOsdDecoder(codes.hamming_code(3), error_rate=0.1, max_iter=5, bp_method="product_sum", osd_method="osd_0")
    with pytest.raises(ValueError, match="same place as the syndromes"):
        d.decode_batch(S, channel_probs=torch.full((4, 7), 0.1, dtype=torch.float64))


@pytest.mark.parametrize("kw, what", [
    (dict(schedule="serial"), "schedule='serial'"),
    (dict(schedule="serial_relative"), "schedule='serial_relative'"),
    (dict(schedule="serial", random_serial_schedule=True, random_schedule_seed=3), "schedule='serial'"),
    (dict(input_vector_type="received_vector"), "received_vector"),
    (dict(device_ids=[0]), "device_ids"),
])
def test_not_implemented(kw, what):
    d = _bp(**kw)
    s = np.ones((4, 7), np.uint8) if "input_vector_type" in kw else S
    with pytest.raises(NotImplementedError, match=what):
        d.decode_batch(s, channel_probs=P)


@pytest.mark.parametrize("method, order", [("osd_e", 3), ("osd_cs", 2), ("osd_e", 0)])
def test_higher_order_osd_is_refused(method, order):
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    d = BpOsdDecoder(codes.hamming_code(3), error_rate=0.1, max_iter=5, bp_method="product_sum", osd_method=method, osd_order=order)
    with pytest.raises(NotImplementedError, match=r"log\(1 / p\)"):
        d.decode_batch(S, channel_probs=P)


def test_soft_info_decoder_refuses():
    from ldpc_amd.bp_decoder import SoftInfoBpDecoder
    d = SoftInfoBpDecoder(codes.hamming_code(3), error_rate=0.1, max_iter=5)
    with pytest.raises(NotImplementedError, match="SoftInfoBpDecoder"):
        d.decode_batch(np.ones((4, 3)), channel_probs=P)


def test_the_keyword_changes_no_existing_call():
    import inspect
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    for cls in (BpDecoder, BpOsdDecoder):
        par = inspect.signature(cls.decode_batch).parameters["channel_probs"]
        assert par.default is None
        assert "UNCHANGED" in cls.decode_batch.__doc__


def test_symbols_are_listed():
    from ldpc_amd import _lib
    for name in ("ldpc_hip_bp_decode_batch_priors", "ldpc_hip_bp_decode_batch_priors_async", "ldpc_hip_bposd0_decode_batch_priors",
                 "ldpc_hip_bposd0_decode_batch_priors_async"):
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.load(), name)
    lib = _lib.load()
    assert lib.ldpc_hip_bp_decode_batch_priors(None, None, 1, None, None, None, None, None) == -1
    assert b"null" in lib.ldpc_hip_last_error()


@pytest.mark.skipif(not os.path.isdir("/root/reference/src_python/ldpc"), reason="the reference is not on this machine")
def test_generator_reproduces_the_committed_fixtures_from_the_reference_itself():
    pytest.importorskip("Cython")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_row_priors.py"), "--check"], capture_output=True, text=True,
                       timeout=1500)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert r.stdout.count("== committed fixture") == len(EXPECTED_CASES) and "DIFFERS" not in r.stdout


def test_the_log_twin_is_the_host_log_on_every_prior_argument():
    """row_priors_kernel forms log((1 - p) / p) with bp_math.h's twin of the host's log.  The check pass only ever hands that routine ratios
    in [2^-54, 2^54]; a prior's ratio ranges over [0, +inf]: 0 (p = 1), 2^-53, 1 (p = 0.5), 1e300, +inf (p = 0 and p below 2^-1024)."""
    import ctypes as C
    from row_priors_util import SPECIAL
    here = os.path.dirname(os.path.abspath(__file__))
    src, so = os.path.join(here, "native", "device_math_host.cpp"), os.path.join(here, "native", "libdevice_math_host.so")
    hdr = os.path.join(ROOT, "ldpc_amd", "csrc", "bp_math.h")
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):  # (as tests/test_device_math.py builds it)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-o", so, src], check=True)
    lib = C.CDLL(so)
    dp = np.ctypeslib.ndpointer(np.float64, flags="C")
    lib.dx_log_v.argtypes = lib.libm_log_v.argtypes = [C.c_long, dp, dp]
    rng = np.random.default_rng(5)
    p = np.concatenate([np.array(SPECIAL), np.array([5e-324, 2.0 ** -1074, 2.0 ** -1030, 2.0 ** -1023, 2.0 ** -1022, 1e-308, 1e-17, np.nextafter(0.5, 0), np.nextafter(0.5, 1),
                                                     np.nextafter(1.0, 0)]),
                        10.0 ** rng.uniform(-320, 0, 200000), rng.random(200000), 1.0 - 10.0 ** rng.uniform(-16, 0, 100000)])
    p = p[(p >= 0) & (p <= 1)]
    with np.errstate(divide="ignore", over="ignore"):
        q = np.ascontiguousarray((1.0 - p) / p)
    got, want = np.zeros_like(q), np.zeros_like(q)
    lib.dx_log_v(len(q), q, got)
    lib.libm_log_v(len(q), q, want)
    assert oracle.bits_equal(got, want), f"{int((got.view(np.uint64) != want.view(np.uint64)).sum())} of {len(q)} priors differ from the host's log"
    assert got[0] == np.inf and got[1] == -np.inf and got[2] == 0.0 and not np.signbit(got[2])
