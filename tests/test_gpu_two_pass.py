"""The streamed two-pass decode (csrc/host_stream.h: decode_stream_repacked, two StreamPass of decode_streamed): first pass k1 iterations, the rows still decoding compacted
lane by lane into dense tiles, a second pass to the end -- against the plain decode (no pass structure at all) and the CPU checker: every row
bit for bit, regular (ring variant) and irregular (per-pass kernels) codes, both methods, with and without log-ratios, a hopeless row, a
partial last tile."""
import numpy as np
import pytest

import launch_util

pytestmark = pytest.mark.gpu


def _decode(eng, s, **kw):
    return [x.cpu().numpy() if x is not None and hasattr(x, "cpu") else x for x in eng.decode_batch(s, **kw)]


@pytest.mark.parametrize("code,method,alpha,p,max_iter", [("ldpc36", 0, 1.0, 0.055, 30), ("ldpc36", 1, 0.8, 0.05, 40), ("irregular", 0, 1.0, 0.035, 24), ("ldpc48", 1, 0.0, 0.04, 30)])
def test_two_pass_decode_gives_the_plain_decodes_bits(code, method, alpha, p, max_iter, oracle_built):
    from golden_util import bits_equal
    from ldpc_amd import codes
    from ldpc_amd.engine import HipBpEngine
    n = 600
    h = {"ldpc36": lambda: codes.regular_ldpc_code(n, 3, 6, seed=3), "ldpc48": lambda: codes.regular_ldpc_code(n, 4, 8, seed=3),
         "irregular": lambda: codes.irregular_ldpc_code(n, n // 2, seed=3)}[code]()
    eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, p), max_iter, method, alpha)
    eng.set_small_code_kernel(0)   # the streamed kernels (what a code beyond LDS takes)
    B = 40000 + 37                 # 626 tiles, the last one partial
    s = eng.gen_bsc_syndromes(5, p, shot0=0, shots=B, device="cuda:0")
    s[777, 3] = 2                  # never converges: in every pass to the end
    eng.set_repack(0)
    ref = _decode(eng, s, want_llr=True)
    assert 0.5 < ref[3].mean() < 0.9999 and ref[2][ref[3].astype(bool)].min() < ref[2][ref[3].astype(bool)].max()
    rows = np.r_[0:50, 770:790, B - 40:B]
    name = "product_sum" if method == 0 else "minimum_sum"
    want = oracle_built.BpOracle(h, error_rate=p, max_iter=max_iter, bp_method=name, ms_scaling_factor=alpha).decode_batch(s.cpu().numpy()[rows])
    assert np.array_equal(ref[0][rows], want[0]) and np.array_equal(ref[2][rows], want[2]) and np.array_equal(ref[3][rows].astype(bool), want[3].astype(bool))
    assert bits_equal(ref[1][rows], want[1])
    for k1 in (2, 3, 5):
        eng.set_repack(k1)
        for want_llr in (True, False):
            with launch_util.launch_log() as log:
                got = _decode(eng, s, want_llr=want_llr)
            tag = (code, method, k1, want_llr)
            launch_util.assert_ran(log, "gather_lane_state_kernel")  # a second pass there was: the rows still decoding were compacted lane by lane
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), tag
            assert got[1] is None if not want_llr else bits_equal(got[1], ref[1]), tag
    # steered by the histogram of the previous decode (repack -1): whatever it chooses, the same bits
    eng.set_repack(-1)
    for _ in range(3):
        got = _decode(eng, s, want_llr=True)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]) and bits_equal(got[1], ref[1])
    eng.close()


def test_second_pass_with_compacted_late_rounds_gives_the_plain_decodes_bits(oracle_built):
    """The late rounds of a second pass (bp_spread_compact_kernel, then 32 + 8 workgroup rows per launch): mild noise, so that the histogram the
    first steered decode leaves shows a handful of stragglers -- here the three hopeless rows and the few that need 13 iterations or more -- and
    the second pass of the next ones compacts its list of parked tiles every 8 rounds.  Every steered decode must equal the plain one bit for bit."""
    from golden_util import bits_equal
    from ldpc_amd import codes
    from ldpc_amd.engine import HipBpEngine
    n, p, max_iter, alpha = 600, 0.03, 40, 0.8
    h = codes.regular_ldpc_code(n, 3, 6, seed=3)
    eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, p), max_iter, 1, alpha)
    eng.set_small_code_kernel(0)
    B = 33000 + 37                 # 517 tiles, the last one partial
    s = eng.gen_bsc_syndromes(5, p, shot0=0, shots=B, device="cuda:0")
    hopeless = [100, 7777, 20011]
    for r in hopeless:
        s[r, 3] = 2
    eng.set_repack(0)
    ref = _decode(eng, s, want_llr=True)
    conv = ref[3].astype(bool)
    print("unconverged rows:", int((~conv).sum()), " mean iterations of the rest:", float(ref[2][conv].mean()))
    # what makes the late rounds compact (host_stream.h: may_compact): at most 24 rows still running late in the second pass
    assert 1 <= (~conv).sum() <= 24 and ref[2][conv].mean() < 8
    rows = np.r_[hopeless, 0:32, B - 32:B]
    want = oracle_built.BpOracle(h, error_rate=p, max_iter=max_iter, bp_method="minimum_sum", ms_scaling_factor=alpha).decode_batch(s.cpu().numpy()[rows])
    assert np.array_equal(ref[0][rows], want[0]) and np.array_equal(ref[2][rows], want[2]) and np.array_equal(conv[rows], want[3].astype(bool))
    assert bits_equal(ref[1][rows], want[1])
    eng.set_repack(-1)
    logs = []
    for i in range(3):  # the first leaves a histogram, the next two are steered by one
        with launch_util.launch_log() as log:
            got = _decode(eng, s, want_llr=True)
        logs.append(log)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]) and bits_equal(got[1], ref[1]), i
    # ... and a steered decode did compact its parked tiles: the kernel this test is about ran
    launch_util.assert_ran(logs[-1], "bp_spread_compact_kernel", "gather_lane_state_kernel")
    eng.close()
