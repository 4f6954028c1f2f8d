"""GPU parity: the HIP path (through the C ABI) against the reference's captured outputs and the oracle.

Bar (BASELINE.json north_star): hard decisions, converge flags and iteration counts bit-exact;
posterior log-probability ratios within 1e-5 RELATIVE.  The kernels do better than the bar: min-sum
has no transcendental and the default product-sum math is a bit-identical twin of the host glibc
the reference runs on (ldpc_amd/csrc/bp_math.h), so against the GOLDEN vectors (captured from the
real reference in the build container) LLRs are asserted BIT-EXACT for both methods.  Against the
oracle, which calls the libm of whatever host runs the test, product-sum LLRs are asserted bit-exact
when that libm is the same glibc and within 1e-5 otherwise.  The optional fast math mode is held
to the north_star tolerance.
Nothing here reads /root/reference; oracle/ is used only as the checker.
"""
import numpy as np
import pytest

import launch_util

from golden_util import bits_equal, case_names, load_case, llr_close, rowsum

pytestmark = pytest.mark.gpu

LLR_RTOL = 1e-5  # north_star tolerance


def _engine(c, **over):
    from ldpc_amd.engine import HipBpEngine
    h = c["h"]
    return HipBpEngine(h.indptr, h.indices, c["n"], over.get("channel_probs", c["channel_probs"]),
                       over.get("max_iter", c["max_iter"]), 0 if c["bp_method"] == "product_sum" else 1,
                       c["ms_scaling_factor"])


def _host_libm_is_glibc():
    import platform
    return platform.machine() == "x86_64" and platform.libc_ver()[0] == "glibc"


def _synd(h, p, seed, shots, shot0=0):
    from ldpc_amd.noise_models import generate_bsc_batch
    err = generate_bsc_batch(h.shape[1], p, seed, shot0, shots)
    return (err.astype(np.int64) @ h.T.toarray().astype(np.int64) % 2).astype(np.uint8)


@pytest.mark.parametrize("name", case_names())
def test_golden_fixture(name):
    """Every fixture captured from the real reference decoder, decoded by the HIP kernels."""
    c = load_case(name)
    eng = _engine(c)
    dec, llr, it, cv = eng.decode_batch(c["syndromes"])
    assert np.array_equal(dec, c["decoding"]), "hard decisions differ from the reference"
    assert np.array_equal(cv, c["converge"]), "converge flags differ from the reference"
    assert np.array_equal(it, c["iterations"]), "iteration counts differ from the reference"
    k = len(c["llr"])
    assert llr_close(llr[:k], c["llr"], rtol=LLR_RTOL)          # the north_star bar
    assert bits_equal(llr[:k], c["llr"]), "LLRs are expected to match the reference bit for bit"
    assert np.allclose(rowsum(llr), c["llr_rowsum"], rtol=1e-12, atol=1e-12)


KNIFE_EDGE = {"edge_degree1_empty_ps"}  # reference posterior exactly 0.0: only the libm-exact mode reproduces it


@pytest.mark.parametrize("name", [n for n in case_names() if n not in KNIFE_EDGE])
def test_golden_fixture_fast_math(name):
    """Optional fast math (ldpc_hip_bp_set_math(1)): exact decisions/flags/iterations, LLRs within 1e-5."""
    c = load_case(name)
    eng = _engine(c)
    eng.set_math("fast")
    dec, llr, it, cv = eng.decode_batch(c["syndromes"])
    assert np.array_equal(dec, c["decoding"])
    assert np.array_equal(cv, c["converge"])
    assert np.array_equal(it, c["iterations"])
    assert llr_close(llr[: len(c["llr"])], c["llr"], rtol=LLR_RTOL)


def test_golden_through_device_pointers():
    """Same call with torch CUDA tensors (device pointers, outputs resident in HBM)."""
    import torch
    c = load_case("c5_bb144_ps50_p050")
    eng = _engine(c)
    s = torch.from_numpy(c["syndromes"]).cuda()
    dec, llr, it, cv = eng.decode_batch(s)
    assert dec.is_cuda and llr.is_cuda
    assert np.array_equal(dec.cpu().numpy(), c["decoding"])
    assert np.array_equal(cv.cpu().numpy().astype(bool), c["converge"])
    assert np.array_equal(it.cpu().numpy(), c["iterations"])
    assert llr_close(llr.cpu().numpy()[: len(c["llr"])], c["llr"], rtol=LLR_RTOL)
    dec2, _, it2, _ = eng.decode_batch(s, want_llr=False)
    assert torch.equal(dec, dec2) and torch.equal(it, it2)


CODES = {
    "ldpc36_n1200": lambda: __import__("ldpc_amd.codes", fromlist=["x"]).regular_ldpc_code(1200, 3, 6, seed=9),
    "surface11": lambda: __import__("ldpc_amd.codes", fromlist=["x"]).rotated_surface_code_x(11),
    "bb144": lambda: __import__("ldpc_amd.codes", fromlist=["x"]).bivariate_bicycle_hx(),
    "hamming6": lambda: __import__("ldpc_amd.codes", fromlist=["x"]).hamming_code(6),  # row weight 32: streaming path
    "ring33": lambda: __import__("ldpc_amd.codes", fromlist=["x"]).ring_code(33),
}


@pytest.mark.parametrize("code,p,max_iter,method,alpha,shots", [
    ("ldpc36_n1200", 0.05, 50, "product_sum", 1.0, 700),
    ("ldpc36_n1200", 0.08, 50, "product_sum", 1.0, 300),
    ("ldpc36_n1200", 0.06, 40, "minimum_sum", 0.625, 700),
    ("ldpc36_n1200", 0.06, 40, "minimum_sum", 0.0, 300),
    ("surface11", 0.04, 30, "minimum_sum", 0.625, 1000),
    ("surface11", 0.04, 30, "product_sum", 1.0, 1000),
    ("bb144", 0.05, 50, "product_sum", 1.0, 1500),
    ("bb144", 0.05, 50, "minimum_sum", 0.9, 1500),
    ("hamming6", 0.03, 25, "product_sum", 1.0, 333),
    ("hamming6", 0.03, 25, "minimum_sum", 0.75, 333),
    ("ring33", 0.1, 33, "product_sum", 1.0, 65),
])
def test_against_oracle_on_seeded_batches(code, p, max_iter, method, alpha, shots, oracle_built):
    """Ragged batch sizes (partial last tile, several tiles), both methods, regular and irregular degrees."""
    from ldpc_amd.engine import HipBpEngine
    h = CODES[code]()
    n = h.shape[1]
    synd = _synd(h, p, seed=1234, shots=shots)
    o = oracle_built.BpOracle(h, error_rate=p, max_iter=max_iter, bp_method=method, ms_scaling_factor=alpha)
    wd, wl, wi, wc = o.decode_batch(synd)
    eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, p), max_iter, 0 if method == "product_sum" else 1, alpha)
    dec, llr, it, cv = eng.decode_batch(synd)
    assert np.array_equal(dec, wd)
    assert np.array_equal(cv, wc)
    assert np.array_equal(it, wi)
    assert llr_close(llr, wl, rtol=LLR_RTOL)
    if method == "minimum_sum" or _host_libm_is_glibc():
        assert bits_equal(llr, wl)
    # property: a converged row reproduces its syndrome (bp.hpp:300-302)
    chk = (dec.astype(np.int64) @ h.T.toarray().astype(np.int64)) % 2
    assert np.array_equal(chk[cv], synd[cv])


@pytest.mark.parametrize("waves", [1, 2, 4, 8, 16])
def test_workgroup_shape_does_not_change_results(waves, oracle_built):
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import regular_ldpc_code
    h = regular_ldpc_code(600, 3, 6, seed=3)
    synd = _synd(h, 0.06, seed=5, shots=130)
    wd, wl, wi, wc = oracle_built.BpOracle(h, error_rate=0.06, max_iter=30).decode_batch(synd)
    eng = HipBpEngine(h.indptr, h.indices, 600, np.full(600, 0.06), 30, 0, 1.0)
    eng.set_tuning(waves_per_workgroup=waves)
    dec, llr, it, cv = eng.decode_batch(synd)
    assert np.array_equal(dec, wd) and np.array_equal(it, wi) and np.array_equal(cv, wc)
    assert llr_close(llr, wl, rtol=LLR_RTOL)


def test_chunked_batches_match_single_launch(oracle_built):
    """Workspace chunking (batch larger than the per-launch tile budget) is invisible in the results."""
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import bivariate_bicycle_hx
    h = bivariate_bicycle_hx()
    synd = _synd(h, 0.05, seed=77, shots=1000)
    eng = HipBpEngine(h.indptr, h.indices, 144, np.full(144, 0.05), 50, 0, 1.0)
    d0, l0, i0, c0 = eng.decode_batch(synd)
    eng.set_tuning(max_chunk_tiles=3)
    d1, l1, i1, c1 = eng.decode_batch(synd)
    assert np.array_equal(d0, d1) and np.array_equal(i0, i1) and np.array_equal(c0, c1)
    assert bits_equal(l0, l1)


@pytest.mark.parametrize("handoff", [-1, 0, 2])
def test_chunked_streaming_kernel_with_handoff(handoff):
    """The streaming path proper (on-chip kernels off) cut into chunks of 3 tiles, with and without parking tiles."""
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import regular_ldpc_code
    h = regular_ldpc_code(600, 3, 6, seed=3)
    synd = _synd(h, 0.06, seed=5, shots=700)  # 11 tiles: chunks of 3, 3, 3, 2
    for method, alpha in ((0, 1.0), (1, 0.75)):
        eng = HipBpEngine(h.indptr, h.indices, 600, np.full(600, 0.06), 40, method, alpha)
        eng.set_small_code_kernel(0)
        eng.set_handoff(0)
        d0, l0, i0, c0 = eng.decode_batch(synd)
        eng.set_handoff(handoff)
        eng.set_tuning(max_chunk_tiles=3)
        d1, l1, i1, c1 = eng.decode_batch(synd)
        assert np.array_equal(d0, d1) and np.array_equal(i0, i1) and np.array_equal(c0, c1)
        assert bits_equal(l0, l1)
        assert 0 < c0.mean() < 1  # both converging and non-converging rows in the batch


def test_batch_independence_and_determinism():
    """Lane/tile position never influences a syndrome's result: permuted and duplicated rows agree."""
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import regular_ldpc_code
    h = regular_ldpc_code(1200, 3, 6, seed=9)
    synd = _synd(h, 0.07, seed=3, shots=500)
    eng = HipBpEngine(h.indptr, h.indices, 1200, np.full(1200, 0.07), 50, 0, 1.0)
    d0, l0, i0, c0 = eng.decode_batch(synd)
    perm = np.random.default_rng(0).permutation(500)
    d1, l1, i1, c1 = eng.decode_batch(synd[perm])
    assert np.array_equal(d0[perm], d1) and np.array_equal(i0[perm], i1) and np.array_equal(c0[perm], c1)
    assert bits_equal(l0[perm], l1)
    d2, l2, i2, c2 = eng.decode_batch(np.repeat(synd[:7], 40, axis=0))
    assert np.array_equal(d2, np.repeat(d0[:7], 40, axis=0))
    assert bits_equal(l2, np.repeat(l0[:7], 40, axis=0))


def test_empty_and_single_row_batches():
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import rep_code
    h = rep_code(5)
    eng = HipBpEngine(h.indptr, h.indices, 5, np.full(5, 0.1), 5, 0, 1.0)
    dec, llr, it, cv = eng.decode_batch(np.zeros((0, 4), np.uint8))
    assert dec.shape == (0, 5) and llr.shape == (0, 5)
    dec, llr, it, cv = eng.decode_batch(np.array([[0, 1, 0, 1]], np.uint8))
    assert dec.tolist() == [[0, 0, 1, 1, 0]]  # TestBPDecoder.cpp:180-186


def test_channel_and_parameter_updates(oracle_built):
    """set_channel / set_params mirror the reference's mutable members (pyx:180-223, 342-394)."""
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import hamming_code
    h = hamming_code(4)
    synd = _synd(h, 0.1, seed=8, shots=100)
    eng = HipBpEngine(h.indptr, h.indices, 15, np.full(15, 0.1), 10, 0, 1.0)
    chan = np.linspace(0.01, 0.3, 15)
    eng.set_channel(chan)
    eng.set_params(7, 1, 0.8)
    wd, wl, wi, wc = oracle_built.BpOracle(h, error_channel=chan, max_iter=7, bp_method="ms",
                                           ms_scaling_factor=0.8).decode_batch(synd)
    dec, llr, it, cv = eng.decode_batch(synd)
    assert np.array_equal(dec, wd) and np.array_equal(it, wi) and np.array_equal(cv, wc)
    assert bits_equal(llr, wl)


def test_device_generator_and_mulvec_match_host_twins(oracle_built):
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import bivariate_bicycle_hx
    from ldpc_amd.noise_models import generate_bsc_batch
    h = bivariate_bicycle_hx()
    eng = HipBpEngine(h.indptr, h.indices, 144, np.full(144, 0.05), 5, 0, 1.0)
    synd, err = eng.gen_bsc_syndromes(7, 0.05, shot0=1000, shots=300, want_errors=True)
    assert np.array_equal(err, generate_bsc_batch(144, 0.05, 7, 1000, 300))
    want = (err.astype(np.int64) @ h.T.toarray().astype(np.int64) % 2).astype(np.uint8)
    assert np.array_equal(synd, want)
    assert np.array_equal(eng.mulvec_batch(err), want)  # gf2sparse.hpp:177-214
    assert np.array_equal(synd, oracle_built.BpOracle(h, error_rate=0.05).gen_bsc_syndromes(7, 0.05, 1000, 300))


def test_full_size_config2_properties():
    """BASELINE config 2 shape at full batch width per tile count that fits a test: (3,6) n=10000, PS-50.

    Size-independent properties: converged rows satisfy H x = s; repeated syndromes decode identically
    wherever they sit; the first rows equal the reference's golden outputs.
    """
    from ldpc_amd.engine import HipBpEngine
    c = load_case("c2_ldpc36_n10000_ps50_p050")
    h = c["h"]
    eng = HipBpEngine(h.indptr, h.indices, 10000, c["channel_probs"], 50, 0, 1.0)
    s = eng.gen_bsc_syndromes(7, 0.05, shot0=0, shots=4096, device="cuda:0")
    s[4000:4012] = s[0:12]
    dec, llr, it, cv = eng.decode_batch(s)
    d = dec.cpu().numpy()
    assert np.array_equal(d[:12], c["decoding"]) and np.array_equal(d[4000:4012], c["decoding"])
    assert np.array_equal(it.cpu().numpy()[:12], c["iterations"])
    assert llr_close(llr[:2].cpu().numpy(), c["llr"], rtol=LLR_RTOL)
    conv = cv.cpu().numpy().astype(bool)
    assert conv.mean() > 0.99
    chk = np.asarray((h.astype(np.int32) @ d.T.astype(np.int32)).T % 2, dtype=np.uint8)
    assert np.array_equal(chk[conv], s.cpu().numpy()[conv])


@pytest.mark.parametrize("method,alpha", [("product_sum", 1.0), ("minimum_sum", 0.625)])
@pytest.mark.parametrize("ring", [0, 2, 3])
def test_kernel_variants_agree_bit_for_bit(method, alpha, ring, oracle_built):
    """LDS-DMA ring (depth 2/3) and register-prefetch variants move data differently but compute identically."""
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import regular_ldpc_code
    h = regular_ldpc_code(1200, 3, 6, seed=9)  # exactly regular -> the ring variant is eligible
    synd = _synd(h, 0.07, seed=21, shots=300)
    wd, wl, wi, wc = oracle_built.BpOracle(h, error_rate=0.07, max_iter=40, bp_method=method,
                                           ms_scaling_factor=alpha).decode_batch(synd)
    eng = HipBpEngine(h.indptr, h.indices, 1200, np.full(1200, 0.07), 40, 0 if method == "product_sum" else 1, alpha)
    eng.set_ring(ring)
    for waves in (0, 4, 16):
        eng.set_tuning(waves_per_workgroup=waves)
        dec, llr, it, cv = eng.decode_batch(synd)
        assert np.array_equal(dec, wd) and np.array_equal(it, wi) and np.array_equal(cv, wc)
        assert llr_close(llr, wl, rtol=LLR_RTOL)
        if method == "minimum_sum" or _host_libm_is_glibc():
            assert bits_equal(llr, wl)


def test_odd_column_count_and_tiny_regular_code(oracle_built):
    """Ring variant edge cases: odd n (last column pair has one member), fewer rows than wavefronts x depth."""
    import scipy.sparse as sp
    from ldpc_amd.engine import HipBpEngine
    # (3,6)-regular with n = 6 * 3 = 18... use circulant construction: n = 9 columns of weight 2? keep (3,6): n=2m
    rng = np.random.default_rng(4)
    m, n = 7, 14  # rows of weight 6, columns of weight 3 via three shifted identity pairs
    rows, cols = [], []
    for i in range(m):
        for t, sft in enumerate((0, 1, 3)):
            rows += [i, i]
            cols += [(i + sft) % m, m + (i + 2 * sft) % m]
    h = sp.csr_matrix((np.ones(len(rows), np.uint8), (rows, cols)), shape=(m, n))
    h.sum_duplicates(); h.data[:] = 1; h.sort_indices()
    assert set(np.diff(h.indptr)) == {6} and set(np.asarray(h.sum(0)).ravel()) == {3}
    synd = rng.integers(0, 2, size=(70, m)).astype(np.uint8)
    for method, alpha in (("product_sum", 1.0), ("minimum_sum", 0.8)):
        wd, wl, wi, wc = oracle_built.BpOracle(h, error_rate=0.08, max_iter=12, bp_method=method,
                                               ms_scaling_factor=alpha).decode_batch(synd)
        eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, 0.08), 12, 0 if method == "product_sum" else 1, alpha)
        for waves in (1, 4, 16):
            eng.set_tuning(waves_per_workgroup=waves)
            dec, llr, it, cv = eng.decode_batch(synd)
            assert np.array_equal(dec, wd) and np.array_equal(it, wi) and np.array_equal(cv, wc)
            assert llr_close(llr, wl, rtol=LLR_RTOL)


def test_bpdecoder_api_matches_reference_known_answers():
    """The reference's own Python tests (python_test/test_bp_decoder.py:175-211), run against the mirror class."""
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.codes import rep_code
    H = rep_code(3)
    bpd = BpDecoder(H, error_rate=0.1, input_vector_type="syndrome")
    assert bpd.bp_method == "product_sum" and bpd.schedule == "parallel"
    assert np.array_equal(bpd.error_channel, np.array([0.1, 0.1, 0.1]))
    bpd.decode(np.array([1, 1]))
    assert np.array_equal(bpd.decoding, np.array([0, 1, 0]))
    bpd.error_channel = np.array([0.1, 0, 0.1])
    bpd.decode(np.array([1, 1]))
    assert np.array_equal(bpd.decoding, np.array([1, 0, 1]))
    ms = BpDecoder(H, error_rate=0.1, bp_method="min_sum", ms_scaling_factor=1.0)
    assert ms.bp_method == "minimum_sum"
    ms.decode(np.array([1, 1]))
    assert np.array_equal(ms.decoding, np.array([0, 1, 0]))
    ms.error_channel = np.array([0.1, 0, 0.1])
    ms.decode(np.array([1, 1]))
    assert np.array_equal(ms.decoding, np.array([1, 0, 1]))


def test_bpdecoder_decode_and_batch_semantics(oracle_built):
    """decode(): dtype preserved, converge/iter/log_prob_ratios properties, received-vector mode, zero shortcut;
    decode_batch(): row b == decode(row b)."""
    from ldpc_amd.bp_decoder import BpDecoder
    c = load_case("c1_hamming5_ps20")
    h = c["h"]
    d = BpDecoder(h, error_rate=0.1, max_iter=20, bp_method="product_sum")
    s = c["syndromes"][3]
    out = d.decode(s.astype(np.int64))
    assert out.dtype == np.int64 and np.array_equal(out, c["decoding"][3])
    assert d.converge == bool(c["converge"][3]) and d.iter == int(c["iterations"][3])
    assert bits_equal(d.log_prob_ratios, c["llr"][3])
    # received-vector mode (bp.hpp:162-180): input of length n -> syndrome = H r, output = bp(H r) XOR r
    r = np.zeros(31, np.uint8); r[[2, 17]] = 1
    got = d.decode(r)
    syn = (h @ r) % 2
    want, _, _, _ = oracle_built.BpOracle(h, error_rate=0.1, max_iter=20).decode_batch(syn[None, :].astype(np.uint8))
    assert np.array_equal(got, want[0] ^ r)
    # all-zero input: zeros, converge=True, BP state untouched (pyx:679-681)
    before = d.log_prob_ratios.copy()
    z = d.decode(np.zeros(5, np.uint8))
    assert not z.any() and d.converge is True and bits_equal(d.log_prob_ratios, before)
    # batch
    batch = d.decode_batch(c["syndromes"])
    nz = c["syndromes"].any(axis=1)
    assert np.array_equal(batch[nz], c["decoding"][nz]) and not batch[~nz].any()
    assert np.array_equal(d.converge_batch[nz], c["converge"][nz]) and d.converge_batch[~nz].all()
    assert np.array_equal(d.iter_batch[nz], c["iterations"][nz])
    with pytest.raises(ValueError):
        d.decode(np.zeros(7, np.uint8))
    # the schedules that keep state in the decoder object run on the device too (tests/test_stateful_schedules.py pins their bits)
    o = oracle_built.BpOracle(h, error_rate=0.1, max_iter=h.shape[1], bp_method="product_sum")
    want = o.decode_serial_relative_batch(s[None, :])
    d = BpDecoder(h, error_rate=0.1, schedule="serial_relative")
    assert np.array_equal(d.decode(s), want[0][0]) and np.array_equal(d.serial_schedule_order, want[4])
    want = o.decode_random_serial_batch(s[None, :], 11)
    assert np.array_equal(BpDecoder(h, error_rate=0.1, schedule="serial", random_schedule_seed=11, random_serial_schedule=True).decode(s), want[0][0])


# ---- BP + OSD-0 (BASELINE config 5) ---------------------------------------

from golden_util import osd_case_names  # noqa: E402


@pytest.mark.parametrize("name", osd_case_names())
def test_bposd0_golden_fixture(name):
    """BpOsdDecoder (OSD_0) outputs captured from the real reference vs ldpc_hip_bposd0_decode_batch."""
    c = load_case(name)
    eng = _engine(c)
    dec, llr, it, cv = eng.decode_batch(c["syndromes"], osd0=True)
    assert np.array_equal(cv, c["converge"]) and np.array_equal(it, c["iterations"])
    assert np.array_equal(dec, c["decoding"]), "BP+OSD-0 decisions differ from the reference"
    chk = (dec.astype(np.int64) @ c["h"].T.toarray().astype(np.int64)) % 2
    assert np.array_equal(chk, c["syndromes"])  # cpp_test/TestOsdDecoder.cpp:9-35
    dec2, _, _, _ = eng.decode_batch(c["syndromes"], want_llr=False, osd0=True)  # library-owned LLR buffer
    assert np.array_equal(dec2, dec)
    status = eng.osd_status(len(dec))
    assert np.array_equal(status, np.where(cv, 0, 1)), "0 = BP converged, 1 = OSD solved H x = s (every fixture syndrome lies in the image)"
    # the register kernel without the column permutation (what matrices beyond 128 x 256 or with rows heavier than eight take), and the
    # rows listed after the BP kernel instead of by it: same decisions, same status
    for switch in ("OSD_NO_FLAT", "OSD_COLLECT_AFTER"):
        eng.set_debug_switch(switch, 1)
        assert np.array_equal(eng.decode_batch(c["syndromes"], want_llr=False, osd0=True)[0], dec), switch
        assert np.array_equal(eng.osd_status(len(dec)), status), switch
        eng.set_debug_switch(switch, -1)
    eng.set_osd_kernel(0)  # the LDS-resident elimination (what larger matrices use)
    assert np.array_equal(eng.decode_batch(c["syndromes"], want_llr=False, osd0=True)[0], dec)
    assert np.array_equal(eng.osd_status(len(dec)), status)


def test_bposd0_config5_batch_and_device_pointers(oracle_built):
    """Config 5 at its batch size: BB [[144,12,12]], product_sum 50 iterations + OSD-0, B = 8192, device resident."""
    import torch
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import bivariate_bicycle_hx
    h = bivariate_bicycle_hx()
    eng = HipBpEngine(h.indptr, h.indices, 144, np.full(144, 0.05), 50, 0, 1.0)
    s = eng.gen_bsc_syndromes(7, 0.05, shot0=0, shots=8192, device="cuda:0")
    dec, llr, it, cv = eng.decode_batch(s, osd0=True)
    d, sh = dec.cpu().numpy(), s.cpu().numpy()
    chk = (d.astype(np.int64) @ h.T.toarray().astype(np.int64)) % 2
    assert np.array_equal(chk, sh), "every BP+OSD-0 output must reproduce its syndrome"
    want, _, wi, wc = oracle_built.BpOracle(h, error_rate=0.05, max_iter=50).bposd0_decode_batch(sh[:1500])
    assert np.array_equal(d[:1500], want) and np.array_equal(cv.cpu().numpy()[:1500].astype(bool), wc)
    assert 0.02 < 1.0 - cv.float().mean().item() < 0.2  # a few percent of the rows needed OSD


def test_bposd_decoder_api():
    """BpOsdDecoder mirror: reference keywords/properties (pyx:54-58, 139-234) and decode semantics (pyx:78-136)."""
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    c = load_case("osd_hamming6_ps10")
    d = BpOsdDecoder(c["h"], error_rate=0.06, max_iter=10, bp_method="product_sum", osd_method="osd_0")
    assert d.osd_method == "OSD_0" and d.osd_order == 0 and d.input_vector_type == "syndrome"
    k = int(np.flatnonzero(~c["converge"])[0])
    out = d.decode(c["syndromes"][k].astype(np.int32))
    assert out.dtype == np.int32 and np.array_equal(out, c["decoding"][k]) and d.converge is False
    assert np.array_equal(d.osd0_decoding, c["decoding"][k]) and np.array_equal(d.osdw_decoding, c["decoding"][k])
    batch = d.decode_batch(c["syndromes"])
    nz = c["syndromes"].any(axis=1)
    assert np.array_equal(batch[nz], c["decoding"][nz])
    with pytest.raises(ValueError):
        BpOsdDecoder(c["h"], error_rate=0.06, osd_method="nope")
    with pytest.raises(ValueError):
        BpOsdDecoder(c["h"], error_rate=0.06, osd_method="osd_0", osd_order=3)
    # OSD_CS takes any order since round 4 (pairs among all k = 57 non-pivot columns; second indices past k are skipped -- the
    # reference writes past its candidate string there): order 65 > k gives what order k gives, and it solves the syndrome
    wide = BpOsdDecoder(c["h"], error_rate=0.06, max_iter=10, bp_method="product_sum", osd_method="osd_cs", osd_order=65).decode(c["syndromes"][k])
    at_k = BpOsdDecoder(c["h"], error_rate=0.06, max_iter=10, bp_method="product_sum", osd_method="osd_cs", osd_order=57).decode(c["syndromes"][k])
    assert np.array_equal(wide, at_k) and np.array_equal((c["h"] @ wide) % 2, c["syndromes"][k])
    # (an absurd order is the same sweep as order k -- the pairs' places in the reference's list do not depend on it -- and must not
    # walk 5e9 pair numbers that name nothing)
    huge = BpOsdDecoder(c["h"], error_rate=0.06, max_iter=10, bp_method="product_sum", osd_method="osd_cs", osd_order=100000).decode(c["syndromes"][k])
    assert np.array_equal(huge, at_k)
    with pytest.raises(NotImplementedError):
        BpOsdDecoder(c["h"], error_rate=0.06, osd_method="osd_e", osd_order=25).decode(c["syndromes"][k])
    with pytest.raises(ValueError):
        d.decode(np.zeros(3, np.uint8))


# ---- higher-order OSD (osd.hpp:119-187) ------------------------------------------

from golden_util import osdw_case_names  # noqa: E402


@pytest.mark.parametrize("name", osdw_case_names())
def test_bposdw_golden_fixture(name):
    """BpOsdDecoder with OSD_E / OSD_CS captured from the real reference vs ldpc_hip_bposd_decode_batch."""
    c = load_case(name)
    eng = _engine(c)
    eng.set_osd(c["osd_method"], c["osd_order"])
    dec, llr, it, cv = eng.decode_batch(c["syndromes"], osd=True)
    assert np.array_equal(cv, c["converge"]) and np.array_equal(it, c["iterations"])
    bad = np.flatnonzero((dec != c["decoding"]).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ from the reference's swept solution (first {bad[:5]})"
    eng.set_osd(c["osd_method"], 0)  # order 0 takes the OSD-0 branch whatever the method (osd.hpp:114)
    assert np.array_equal(eng.decode_batch(c["syndromes"], want_llr=False, osd=True)[0], c["osd0_decoding"])
    eng.set_osd(1, 0)
    assert np.array_equal(eng.decode_batch(c["syndromes"], want_llr=False, osd=True)[0], c["osd0_decoding"])
    eng.set_osd_kernel(0)
    eng.set_osd(c["osd_method"], c["osd_order"])
    assert np.array_equal(eng.decode_batch(c["syndromes"], want_llr=False, osd=True)[0], c["decoding"])


@pytest.mark.parametrize("name", ["osdw_cs10_hgp1600_ms12", "osdw_e6_hgp1600_ms12", "osdw_cs8_random400x900_ps6", "osdw_cs10_bb144_ps8",
                                  "osdw_cs64_bb144_ms8", "osdw_e13_hamming4_ps2", "osdw_cs100_hgp1600_ms12", "osdw_cs78_bb144_ps8",
                                  "osdw_cs70_bb144_nonuniform", "osdw_cs90_random120x600_ps4"])
@pytest.mark.parametrize("unblocked", [False, True])
def test_workgroup_osd_kernel_variants(name, unblocked, monkeypatch):
    """osd_big_kernel in each of its forms -- working copy in an HBM slot (osd_kernel 2) or in LDS, blocked elimination or the
    one-pivot-per-step loop matrices with more than 1024 rows take (LDPC_HIP_OSD_UNBLOCKED) -- against the reference's fixtures,
    OSD-0 and the higher order.  (The default dispatch gives small matrices to the one-wavefront kernels.)"""
    c = load_case(name)
    eng = _engine(c)
    if unblocked:
        eng.set_debug_switch("OSD_UNBLOCKED", 1)
    for kernel in (2, -1):  # 2: workgroup kernel, H in HBM whatever the size; -1: the default dispatch (400 x 900: workgroup kernel, copy in LDS)
        eng.set_osd_kernel(kernel)
        eng.set_osd(c["osd_method"], c["osd_order"])
        with launch_util.launch_log() as log_w:
            dec, _, it, cv = eng.decode_batch(c["syndromes"], want_llr=False, osd=True)
        assert np.array_equal(cv, c["converge"]) and np.array_equal(it, c["iterations"])
        assert np.array_equal(dec, c["decoding"]), (kernel, unblocked)
        eng.set_osd(1, 0)
        with launch_util.launch_log() as log_0:
            assert np.array_equal(eng.decode_batch(c["syndromes"], want_llr=False, osd=True)[0], c["osd0_decoding"]), (kernel, unblocked)
        # osd_big_kernel<HIGHER, MAT_LDS>: forced (2), the working copy of H stays in its HBM slot; the 400 x 900 matrix takes it by default, copy in LDS
        mat_lds = "false" if kernel == 2 else "true" if "random400x900" in name else None
        if mat_lds:
            assert launch_util.of(log_w, "osd_big_kernel") == [f"osd_big_kernel<true, {mat_lds}>"], (kernel, sorted(log_w))
            assert launch_util.of(log_0, "osd_big_kernel") == [f"osd_big_kernel<false, {mat_lds}>"], (kernel, sorted(log_0))


@pytest.mark.parametrize("planes", ["1", "2", "4"])
@pytest.mark.parametrize("name", ["osdw_cs10_hgp1600_ms12", "osdw_e6_hgp1600_ms12", "osdw_cs8_random400x900_ps6", "osdw_cs100_hgp1600_ms12",
                                  "osdw_cs90_random120x600_ps4"])
def test_workgroup_osd_kernel_staged_planes(name, planes, monkeypatch):
    """The workgroup kernel weighs candidates with one, two or four wavefronts (one staged T plane each; fewer where LDS would
    otherwise cost resident workgroups and many rows wait): the same solutions whichever it picks."""
    c = load_case(name)
    eng = _engine(c)
    eng.set_debug_switch("OSD_PLANES", int(planes))
    eng.set_osd_kernel(2)
    eng.set_osd(c["osd_method"], c["osd_order"])
    with launch_util.launch_log() as log:
        dec = eng.decode_batch(c["syndromes"], want_llr=False, osd=True)[0]
    assert np.array_equal(dec, c["decoding"])
    assert launch_util.of(log, "osd_big_kernel") == ["osd_big_kernel<true, false>"], sorted(log)


def test_bposdw_device_pointers_and_oracle_at_batch(oracle_built):
    """Config-5 code, OSD_CS order 10 (the setting most BP+OSD papers use), B = 4096 device resident vs the CPU oracle."""
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import bivariate_bicycle_hx
    h = bivariate_bicycle_hx()
    eng = HipBpEngine(h.indptr, h.indices, 144, np.full(144, 0.06), 30, 0, 1.0)
    eng.set_osd(3, 10)
    s = eng.gen_bsc_syndromes(7, 0.06, shot0=0, shots=4096, device="cuda:0")
    dec, llr, it, cv = eng.decode_batch(s, osd=True)
    d, sh = dec.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal((d.astype(np.int64) @ h.T.toarray().astype(np.int64)) % 2, sh)
    want, _, wi, wc = oracle_built.BpOracle(h, error_rate=0.06, max_iter=30).bposd_decode_batch(sh[:768], 3, 10)
    assert np.array_equal(d[:768], want) and np.array_equal(cv.cpu().numpy()[:768].astype(bool), wc)
    with pytest.raises(Exception, match="osd_order"):
        eng.set_osd(2, 25)   # OSD_E: 2^25 candidates per syndrome
    eng.set_osd(3, 65)       # OSD_CS: any order since round 4 (the pairs reach past the first 64 non-pivot columns)
    wide = eng.decode_batch(s[:256].contiguous(), want_llr=False, osd=True)[0].cpu().numpy()
    assert np.array_equal(wide, oracle_built.BpOracle(h, error_rate=0.06, max_iter=30).bposd_decode_batch(sh[:256], 3, 65, want_llr=False)[0])
    with pytest.raises(Exception, match="OSD_0"):
        eng.set_osd(1, 2)


@pytest.mark.parametrize("method", ["minimum_sum", "product_sum"])
def test_team_form_after_a_syndrome_that_ran_out_of_iterations(method, oracle_built):
    """A team decodes one syndrome after another: one that stops at an ODD iteration limit without converging leaves its
    'unsatisfied' flag raised, and the next one may converge in its very first iteration -- many such pairs through few teams."""
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import bivariate_bicycle_hx
    h = bivariate_bicycle_hx()
    m, n = h.shape
    rng = np.random.default_rng(11)
    rows = 40000
    s = np.zeros((rows, m), np.uint8)
    s[0::2] = 2  # a syndrome byte above 1 can never be matched (bp.hpp:300): every other row runs out of iterations
    one = np.zeros((rows // 2, n), np.uint8)
    one[np.arange(rows // 2), rng.integers(0, n, rows // 2)] = 1
    s[1::2] = (one @ h.T.toarray()) % 2  # a single error: converges at once
    for max_iter in (3, 4):
        eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, 0.01), max_iter, 0 if method == "product_sum" else 1, 0.9)
        o = oracle_built.BpOracle(h, error_rate=0.01, max_iter=max_iter, bp_method=method, ms_scaling_factor=0.9)
        want = o.decode_batch(s[:64])
        for small in (5, 1):  # the lane = node kernel as a team; whatever mode 1 picks (product-sum: the lane = entry kernel, a team at this batch size)
            eng.set_small_code_kernel(small)
            dec, llr, it, cv = eng.decode_batch(s, want_llr=False)
            assert np.array_equal(it[0::2], np.full(rows // 2, max_iter)) and not cv[0::2].any()
            assert cv[1::2].all()
            assert int(it[1::2].max()) == int(want[2][1::2].max()) == 1, (small, max_iter)
            assert np.array_equal(dec[:64], want[0])


@pytest.mark.parametrize("name", ["hgp1600_ms20_p030", "hgp1600_ps12_p030"])
@pytest.mark.parametrize("small", [-1, 4, 5, 0])
def test_mid_size_code_one_wavefront_or_a_workgroup_per_syndrome(name, small):
    """768 x 1600: the message array of a syndrome is 49 KiB of LDS, two fit a compute unit.  Automatic = a workgroup per
    syndrome (bp_wave_kernel's TEAM form), 4 = one wavefront per syndrome, 0 = streamed: the reference's bits from each."""
    c = load_case(name)
    eng = _engine(c)
    eng.set_small_code_kernel(small)
    dec, llr, it, cv = eng.decode_batch(c["syndromes"])
    assert np.array_equal(dec, c["decoding"]) and np.array_equal(cv, c["converge"]) and np.array_equal(it, c["iterations"])
    assert bits_equal(llr[: len(c["llr"])], c["llr"])
    d2 = eng.decode_batch(c["syndromes"], want_llr=False)
    assert np.array_equal(d2[0], c["decoding"]) and np.array_equal(d2[2], c["iterations"])


@pytest.mark.parametrize("backend", ["cython", "ctypes"])
def test_bposd_decoder_api_higher_order(backend):
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    c = load_case("osdw_cs10_bb144_ps8")
    d = BpOsdDecoder(c["h"], error_rate=0.08, max_iter=8, bp_method="product_sum", osd_method="osd_cs", osd_order=10,
                     _backend=backend)
    assert d.osd_method == "OSD_CS" and d.osd_order == 10
    rows = np.flatnonzero((c["decoding"] != c["osd0_decoding"]).any(axis=1))[:3]
    for k in rows:
        out = d.decode(c["syndromes"][k])
        assert np.array_equal(out, c["decoding"][k]) and d.converge is False
        assert np.array_equal(d.osdw_decoding, c["decoding"][k])
        assert np.array_equal(d.osd0_decoding, c["osd0_decoding"][k])
    batch = d.decode_batch(c["syndromes"])
    nz = c["syndromes"].any(axis=1)
    assert np.array_equal(batch[nz], c["decoding"][nz])
    d.osd_method = "osd_e"
    d.osd_order = 8
    e = load_case("osdw_e8_bb144_ps8")
    assert np.array_equal(d.decode_batch(e["syndromes"])[e["syndromes"].any(axis=1)], e["decoding"][e["syndromes"].any(axis=1)])


@pytest.mark.parametrize("name", ["c5_bb144_ps50_p050", "c5_bb144_ms50_p050", "c3_surface21_ms30_p050", "surface5_ps30",
                                  "edge_extreme_priors_ps", "edge_syndrome_bytes_gt1_ms", "edge_degree1_empty_ps",
                                  "c1_hamming5_ps20", "ldpc36_n600_ps50_p070"])
@pytest.mark.parametrize("small", [0, 1, 2, 3, 4, 5])  # 4 / 5: the lane = node kernel with one wavefront / a whole workgroup per syndrome
def test_on_chip_and_streaming_kernels_agree_with_the_reference(name, small, monkeypatch):
    """Small codes are decoded by the LDS-resident kernel (auto); forcing either kernel gives the reference's bits."""
    c = load_case(name)
    eng = _engine(c)
    eng.set_small_code_kernel(small)
    dec, llr, it, cv = eng.decode_batch(c["syndromes"])
    assert np.array_equal(dec, c["decoding"]) and np.array_equal(cv, c["converge"]) and np.array_equal(it, c["iterations"])
    assert bits_equal(llr[: len(c["llr"])], c["llr"])
    k = len(c["syndromes"])
    reps = 3001 // k + 2
    big = np.tile(c["syndromes"], (reps, 1))[:3001]  # many more syndromes than resident slots: exercises the work queue
    d2, l2, i2, c2 = eng.decode_batch(big)
    for r in range(0, 3001 - k, k):
        assert np.array_equal(d2[r:r + k], c["decoding"]) and np.array_equal(i2[r:r + k], c["iterations"])
    if small == 1 and c["bp_method"] == "product_sum":  # the lane = entry kernel in both of its forms, whatever the batch size would pick
        for form in ("0", "1"):
            eng.set_debug_switch("PS_TEAM", int(form))
            d3, l3, i3, c3 = eng.decode_batch(c["syndromes"])
            assert np.array_equal(d3, c["decoding"]) and np.array_equal(i3, c["iterations"]) and bits_equal(l3[: len(c["llr"])], c["llr"]), form


@pytest.mark.parametrize("backend", ["cython", "ctypes"])
def test_bpdecoder_backends_give_reference_results(backend):
    """BpDecoder on the Cython binding of the C++ host class and on the ctypes engine: same C ABI, same bits."""
    from ldpc_amd.bp_decoder import BpDecoder
    if backend == "cython":
        pytest.importorskip("ldpc_amd.bp_decoder._bp_core")
    c = load_case("ldpc36_n600_ps50_p070")
    d = BpDecoder(c["h"], error_rate=0.07, max_iter=50, bp_method="product_sum", input_vector_type="syndrome", _backend=backend)
    out = d.decode_batch(c["syndromes"])
    nz = c["syndromes"].any(axis=1)
    assert np.array_equal(out[nz], c["decoding"][nz])
    assert np.array_equal(d.iter_batch[nz], c["iterations"][nz]) and np.array_equal(d.converge_batch[nz], c["converge"][nz])
    k = len(c["llr"])
    assert bits_equal(d.log_prob_ratios_batch[:k][nz[:k]], c["llr"][nz[:k]])
    one = d.decode(c["syndromes"][1])
    assert np.array_equal(one, c["decoding"][1]) and d.iter == int(c["iterations"][1])
    d.error_channel = np.full(600, 0.04)  # setters reach the device object through either binding
    d.max_iter = 7
    c2 = load_case("ldpc36_n600_ps50_p040")
    out2 = d.decode_batch(c2["syndromes"])
    ref_it = np.minimum(c2["iterations"], 7)
    assert np.array_equal(d.iter_batch[c2["syndromes"].any(axis=1)], ref_it[c2["syndromes"].any(axis=1)])


def test_cpp_host_class_demo_runs():
    """examples/cpp_host_demo (pure C++ over include/ldpc_hip.hpp, no Python): the reference's known answers."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "cpp_host_demo")
    if not os.path.exists(exe):
        pytest.skip("examples/cpp_host_demo not built")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


# ---- serial schedule with a fixed bit order (bp.hpp:451-545) ----------------------

from golden_util import serial_case_names  # noqa: E402


@pytest.mark.parametrize("name", serial_case_names())
def test_serial_schedule_golden_fixture(name):
    """Outputs of the real reference's bp_decode_serial (default and custom serial_schedule_order)."""
    c = load_case(name)
    eng = _engine(c)
    eng.set_schedule("serial", c.get("order"))
    for serial_kernel in (-1, 0, 1, 2):  # automatic, bit by bit, level-parallel, streamed (where the matrix allows it)
        eng.set_serial_kernel(serial_kernel)
        dec, llr, it, cv = eng.decode_batch(c["syndromes"])
        assert np.array_equal(dec, c["decoding"]) and np.array_equal(cv, c["converge"]) and np.array_equal(it, c["iterations"])
        assert bits_equal(llr[: len(c["llr"])], c["llr"])
    eng.set_schedule("parallel")  # and back: the flooding schedule is unaffected
    d2, _, i2, _ = eng.decode_batch(c["syndromes"][:8])
    assert d2.shape == (8, c["n"])


def test_serial_schedule_through_bpdecoder(oracle_built):
    """python_test/test_bp_decoder.py:214-235 (rep code, serial schedule, reversed order) + batch vs the oracle."""
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.codes import rep_code, regular_ldpc_code
    H = rep_code(3)
    bpd = BpDecoder(H, error_rate=0.1, schedule="serial")
    assert bpd.schedule == "serial" and np.array_equal(bpd.serial_schedule_order, np.array([0, 1, 2]))
    bpd.serial_schedule_order = np.array([2, 1, 0])
    bpd.decode(np.array([1, 1]))
    assert np.array_equal(bpd.decoding, np.array([0, 1, 0]))
    bpd.error_channel = np.array([0.1, 0, 0.1])
    bpd.decode(np.array([1, 1]))
    assert np.array_equal(bpd.decoding, np.array([1, 0, 1]))
    h = regular_ldpc_code(600, 3, 6, seed=3)
    synd = _synd(h, 0.07, seed=17, shots=200)
    order = np.random.default_rng(2).permutation(600).astype(np.int32)
    d = BpDecoder(h, error_rate=0.07, max_iter=25, bp_method="minimum_sum", ms_scaling_factor=0.8, schedule="serial",
                  serial_schedule_order=[int(v) for v in order], input_vector_type="syndrome")
    out = d.decode_batch(synd)
    wd, wl, wi, wc = oracle_built.BpOracle(h, error_rate=0.07, max_iter=25, bp_method="ms",
                                           ms_scaling_factor=0.8).decode_serial_batch(synd, order)
    nz = synd.any(axis=1)
    assert np.array_equal(out[nz], wd[nz]) and np.array_equal(d.iter_batch[nz], wi[nz])
    assert bits_equal(d.log_prob_ratios_batch[nz], wl[nz])


# ---- straggler hand-off (persistent kernel -> chip-wide per-pass kernels) -----------------------------------

@pytest.mark.parametrize("threshold", [0, 1, 3, 100000])
@pytest.mark.parametrize("code,method,alpha,p,max_iter", [
    ("ldpc36_n1200", "product_sum", 1.0, 0.075, 40),   # ring variant; some syndromes converge, some never do
    ("ldpc36_n1200", "minimum_sum", 0.0, 0.06, 30),    # adaptive alpha depends on the per-tile iteration counter
    ("hamming6", "product_sum", 1.0, 0.03, 25),        # irregular, heavy rows: register variant + streamed rows
])
def test_handoff_gives_identical_results(code, method, alpha, p, max_iter, threshold, oracle_built):
    """Parking tiles after any number of iterations and finishing them with the per-pass kernels changes nothing:
    decisions, flags, iteration counts and LLR bits equal the oracle's for every threshold (0 = never park,
    100000 = every tile parks after its first iteration)."""
    from ldpc_amd.engine import HipBpEngine
    h = CODES[code]()
    n = h.shape[1]
    synd = _synd(h, p, seed=4321, shots=650)
    synd[5, 0] = 2  # a syndrome byte > 1: that lane can never converge (bp.hpp:300)
    wd, wl, wi, wc = oracle_built.BpOracle(h, error_rate=p, max_iter=max_iter, bp_method=method,
                                           ms_scaling_factor=alpha).decode_batch(synd)
    eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, p), max_iter, 0 if method == "product_sum" else 1, alpha)
    eng.set_small_code_kernel(0)
    eng.set_handoff(threshold)
    dec, llr, it, cv = eng.decode_batch(synd)
    assert np.array_equal(dec, wd) and np.array_equal(cv, wc) and np.array_equal(it, wi)
    assert llr_close(llr, wl, rtol=LLR_RTOL)
    if method == "minimum_sum" or _host_libm_is_glibc():
        assert bits_equal(llr, wl)
    dec2, _, it2, _ = eng.decode_batch(synd, want_llr=False)
    assert np.array_equal(dec2, wd) and np.array_equal(it2, wi)


def test_single_syndrome_latency_path_matches_golden():
    """B = 1 on the big code: one tile, parked after the first iteration, finished by the per-pass kernels."""
    from ldpc_amd.engine import HipBpEngine
    c = load_case("c2_ldpc36_n10000_ps50_p090")
    eng = _engine(c)
    for k in range(3):
        dec, llr, it, cv = eng.decode_batch(c["syndromes"][k:k + 1])
        assert np.array_equal(dec[0], c["decoding"][k]) and int(it[0]) == int(c["iterations"][k])
        if k < len(c["llr"]):
            assert bits_equal(llr[0], c["llr"][k])


def test_bpdecoder_decode_batch_device_tensors():
    """decode_batch on torch CUDA tensors (syndromes and received vectors), including the all-zero shortcut rows."""
    import torch
    from ldpc_amd.bp_decoder import BpDecoder
    c = load_case("c1_hamming5_ps20")
    d = BpDecoder(c["h"], error_channel=c["channel_probs"], max_iter=c["max_iter"], bp_method=c["bp_method"])
    s = np.concatenate([c["syndromes"], np.zeros((3, c["m"]), np.uint8)])
    want = d.decode_batch(s)
    st = torch.from_numpy(s).cuda()
    got = d.decode_batch(st)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert bool(d.converge_batch[-3:].all()) and int(d.iter_batch[-3:].abs().sum()) == 0
    assert float(d.log_prob_ratios_batch[-3:].abs().sum()) == 0.0
    rng = np.random.default_rng(4)
    r = (rng.random((40, c["n"])) < 0.04).astype(np.uint8)
    r[5] = 0
    drv = BpDecoder(c["h"], error_rate=0.04, max_iter=20, input_vector_type="received_vector")
    assert np.array_equal(drv.decode_batch(torch.from_numpy(r).cuda()).cpu().numpy(), drv.decode_batch(r))


@pytest.mark.parametrize("first_pass", [-1, 0, 1, 3, 49])
def test_serial_repacking_gives_identical_results(first_pass, oracle_built):
    """Serial schedule with the two-pass repacking (ldpc_hip_bp_set_repack): same bits as one pass and as the oracle."""
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import bivariate_bicycle_hx
    h = bivariate_bicycle_hx()
    synd = _synd(h, 0.06, seed=21, shots=1500)
    for method, alpha in ((0, 1.0), (1, 0.625)):
        eng = HipBpEngine(h.indptr, h.indices, 144, np.full(144, 0.06), 50, method, alpha)
        eng.set_schedule("serial")
        eng.set_repack(0)
        eng.set_serial_kernel(0 if first_pass == 3 else -1)
        d0, l0, i0, c0 = eng.decode_batch(synd)
        eng.set_repack(first_pass)
        d1, l1, i1, c1 = eng.decode_batch(synd)
        assert np.array_equal(d0, d1) and np.array_equal(i0, i1) and np.array_equal(c0, c1) and bits_equal(l0, l1)
        d2, l2, i2, c2 = eng.decode_batch(synd, want_llr=False)
        assert l2 is None and np.array_equal(d2, d0) and np.array_equal(i2, i0)
        eng.set_osd(3, 4)
        d3 = eng.decode_batch(synd, osd=True)[0]
        eng.set_repack(0)
        assert np.array_equal(d3, eng.decode_batch(synd, osd=True)[0])
        assert 0.02 < 1 - c0.mean() < 0.9
    want = oracle_built.BpOracle(h, error_rate=0.06, max_iter=50, bp_method="minimum_sum", ms_scaling_factor=0.625).decode_serial_batch(synd[:300], None)
    assert np.array_equal(d1[:300], want[0]) and np.array_equal(i1[:300], want[2])


@pytest.mark.parametrize("dv,dc", [(4, 8), (2, 4), (3, 9), (5, 10)])
def test_streaming_variants_for_other_regular_codes(dv, dc, oracle_built):
    """(4,8)-regular takes the second LDS-ring instantiation, (2,4) the <4,3> register bounds, (3,9) / (5,10) the
    register variants with wider bounds: every template family of the streaming kernel against the oracle."""
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.codes import regular_ldpc_code
    n = 720
    h = regular_ldpc_code(n, dv, dc, seed=11)
    synd = _synd(h, 0.03, seed=4, shots=200)
    for method, alpha in (("product_sum", 1.0), ("minimum_sum", 0.8)):
        want = oracle_built.BpOracle(h, error_rate=0.03, max_iter=12, bp_method=method, ms_scaling_factor=alpha).decode_batch(synd)
        eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, 0.03), 12, 0 if method == "product_sum" else 1, alpha)
        eng.set_small_code_kernel(0)
        for handoff, ring in ((0, 1), (0, 0), (100000, 1)):
            eng.set_handoff(handoff)
            eng.set_ring(ring)
            got = eng.decode_batch(synd)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
            assert bits_equal(got[1], want[1])


# ---- every output element is written (the result arrays are np.empty / torch.empty: ADVICE round 4) ------------------------------------

def _poisoned_outputs(b, n):
    import torch
    dec = torch.full((b, n), 0xAB, dtype=torch.uint8, device="cuda")
    llr = torch.full((b, n), -1.2345678e300, dtype=torch.float64, device="cuda")  # (NaN would not do: inf - inf is a legitimate log-ratio)
    it = torch.full((b,), -12345, dtype=torch.int32, device="cuda")
    cv = torch.full((b,), 0xAB, dtype=torch.uint8, device="cuda")
    return dec, llr, it, cv


# the kernels that make each path of test_no_output_element_is_left_unwritten what it is called (a tuple: either -- the levels of the shuffled orders decide)
_PATH_KERNELS = {
    "streamed": ["bp_decode_kernel"], "streamed_two_pass": ["bp_decode_kernel", "gather_lane_state_kernel"], "spread": ["bp_spread_check_kernel", "bp_spread_bit_kernel"],
    "wave_ps": ["bp_wave_ps_kernel"], "edge": ["bp_edge_kernel"], "edge8": ["bp_edge8_kernel"], "wave": ["bp_wave_kernel"], "small": ["bp_small_kernel"],
    "serial_level": ["bp_serial_level_kernel"], "serial_walk": ["bp_serial_kernel"], "serial_stream": ["bp_serial_stream_kernel"],
    "serial_lanes": ["bp_serial_lane_kernel"], "serial_relative": ["bp_relative_lds_kernel"], "serial_relative_per_lane": ["bp_serial_relative_kernel"],
    "random_serial": [("bp_serial_level_kernel", "bp_serial_kernel")], "osd0": ["osd0_flat_kernel"], "osd_cs": ["osdw_reg_kernel"],
}


@pytest.mark.parametrize("path", ["streamed", "streamed_two_pass", "spread", "wave_ps", "edge", "edge8", "wave", "small", "serial_level", "serial_walk", "serial_stream",
                                  "serial_lanes", "serial_relative", "serial_relative_per_lane", "random_serial", "osd0", "osd_cs"])
def test_no_output_element_is_left_unwritten(path):
    """Outputs pre-filled with a poison pattern come back without it on every kernel path (a path that skipped rows would hand out
    uninitialised memory: the result arrays are not zero-filled).  The launch log shows that the path's kernel did run."""
    import torch
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd import codes
    cfg = {
        "streamed": (codes.regular_ldpc_code(1200, 3, 6, seed=3), 0.07, 12, 0, 1.0, 70000),
        "streamed_two_pass": (codes.regular_ldpc_code(1200, 3, 6, seed=3), 0.04, 30, 0, 1.0, 40000),
        "spread": (codes.regular_ldpc_code(1200, 3, 6, seed=3), 0.07, 12, 0, 1.0, 333),
        "wave_ps": (codes.bivariate_bicycle_hx(), 0.05, 20, 0, 1.0, 1000),
        "edge": (codes.rotated_surface_code_x(9), 0.05, 15, 1, 0.625, 1000),
        "edge8": (codes.bivariate_bicycle_hx(), 0.05, 20, 1, 0.8, 1000),  # (min-sum on BB144 by default: what "wave" ran until the launch log showed it)
        "wave": (codes.bivariate_bicycle_hx(), 0.05, 20, 1, 0.8, 1000),
        "small": (codes.hamming_code(6), 0.03, 10, 0, 1.0, 300),
        "serial_level": (codes.bivariate_bicycle_hx(), 0.06, 20, 0, 1.0, 1000),
        "serial_walk": (codes.bivariate_bicycle_hx(), 0.06, 20, 1, 0.7, 1000),
        "serial_stream": (codes.regular_ldpc_code(1800, 3, 6, seed=9), 0.07, 20, 0, 1.0, 5000),
        "serial_lanes": (codes.regular_ldpc_code(1800, 3, 6, seed=9), 0.07, 20, 1, 0.8, 77),
        "serial_relative": (codes.bivariate_bicycle_hx(), 0.06, 12, 0, 1.0, 700),
        "serial_relative_per_lane": (codes.bivariate_bicycle_hx(), 0.06, 12, 1, 0.8, 300),
        "random_serial": (codes.bivariate_bicycle_hx(), 0.06, 12, 0, 1.0, 500),
        "osd0": (codes.bivariate_bicycle_hx(), 0.06, 10, 0, 1.0, 900),
        "osd_cs": (codes.bivariate_bicycle_hx(), 0.06, 10, 1, 0.625, 900),
    }[path]
    h, p, max_iter, method, alpha, b = cfg
    m, n = h.shape
    eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, p), max_iter, method, alpha)
    kw = {}
    if path in ("streamed", "streamed_two_pass", "spread"):
        eng.set_small_code_kernel(0)
    if path == "small":
        eng.set_small_code_kernel(2)
    if path == "wave":
        eng.set_small_code_kernel(3)  # the lane = node kernel: by default min-sum on this code takes bp_edge8_kernel (path "edge8")
    if path.startswith("serial_") and not path.startswith("serial_relative"):
        eng.set_schedule("serial")
        eng.set_serial_kernel({"serial_level": 1, "serial_walk": 0, "serial_stream": 2, "serial_lanes": 2}[path])
    if path.startswith("serial_relative"):
        eng.set_schedule("serial_relative")
        if path.endswith("per_lane"):
            eng.set_debug_switch("REL_LDS", 0)
    if path == "random_serial":
        eng.set_schedule("serial")
        eng.set_random_serial(True, 5)
    if path == "osd0":
        kw["osd0"] = True
    if path == "osd_cs":
        eng.set_osd(3, 5)
        kw["osd"] = True
    s = eng.gen_bsc_syndromes(3, p, shot0=0, shots=b, device="cuda:0")
    for rep in range(2):  # (the second call of the streamed path is steered by the first one's histogram: two passes)
        out = _poisoned_outputs(b, n)
        with launch_util.launch_log() as log:
            dec, llr, it, cv = eng.decode_batch(s, out=out, **kw)
        torch.cuda.synchronize()
        if path != "streamed_two_pass" or rep == 1:
            for kernel in _PATH_KERNELS[path]:  # (a tuple: any of them)
                assert launch_util.of(log, *((kernel,) if isinstance(kernel, str) else kernel)), (path, kernel, sorted(log))
            launch_util.assert_resolved(log)
        assert int((dec > 1).sum()) == 0, path
        assert int((cv > 1).sum()) == 0, path
        assert int((it < 0).sum()) == 0 and int((it > max(max_iter, 0)).sum()) == 0, path
        assert int((llr == -1.2345678e300).sum()) == 0, path
    eng.close()
