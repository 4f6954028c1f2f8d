"""Memory min-sum, Relay-BP and guided decimation on ONE handle, which holds at most one of them (``ldpc_hip_bp::variant``): in all six orders of
two, the second setter is refused with the exclusion sentence of ldpc_amd/csrc/mode_host.h, the getters still answer for the first, and the
first decodes to the same bits after the refused call as before it.  Hamming(7,4), 70 syndromes, the lane = edge kernels."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import f32_util as fu
import mem_bp_util as mu
from oracle import bits_equal

pytestmark = pytest.mark.gpu

# label, what to switch off, the call that does it -- as the C messages spell them
SPELLING = {"memory": ("memory min-sum", "the memory", "ldpc_hip_bp_set_memory(h, NULL)"),
            "relay": ("Relay-BP", "the relay", "ldpc_hip_bp_set_relay(h, 0, NULL, NULL, 0)"),
            "decimation": ("guided decimation", "the decimation", "ldpc_hip_bp_set_decimation(h, 0, 0, 0)")}


def test_a_second_variant_is_refused_and_the_first_decodes_on():
    from ldpc_amd import _lib
    from ldpc_amd.engine import HipBpEngine
    c = fu.small_case("hamming3", 0.625)
    h, n = sp.csr_matrix(c["h"]), c["h"].shape[1]
    gamma = mu.mixed_gamma(c["probs"])  # (strength 0 on the columns with p = 0 or 1: nothing for a decode to refuse)
    legs = np.stack([gamma, -0.5 * gamma, 0.5 * gamma])
    settings = {"memory": (gamma,), "relay": (legs, np.array([4, 3, 5], np.int32), 2), "decimation": (2, n + 1, 25.0)}
    eng = HipBpEngine(h.indptr, h.indices, n, c["probs"], c["max_iter"], 1, c["alpha"])
    setters = {"memory": eng.set_memory, "relay": eng.set_relay, "decimation": eng.set_decimation}

    def held():
        return {"memory": eng.memory() is not None, "relay": eng.relay is not None, "decimation": eng.decimation is not None}
    try:
        plain = eng.decode_batch(c["synd"])
        results = {}
        for first, second in itertools.permutations(SPELLING, 2):
            setters[first](*settings[first])
            assert held() == {name: name == first for name in SPELLING}
            before = eng.decode_batch(c["synd"])
            with pytest.raises(_lib.LdpcHipError, match="error -4"):
                setters[second](*settings[second])
            (label, _, _), (other, noun, off) = SPELLING[second], SPELLING[first]
            assert eng._lib.ldpc_hip_last_error().decode() == f"{label} and {other} exclude each other: switch {noun} off first ({off})"
            assert held() == {name: name == first for name in SPELLING}, f"{second} after {first}: the refused setter changed what the handle holds"
            after = eng.decode_batch(c["synd"])
            for k, name in ((0, "decoding"), (2, "iterations"), (3, "converge")):
                assert np.array_equal(after[k], before[k]), f"{second} refused after {first}: {name} changed"
            assert bits_equal(after[1], before[1]), f"{second} refused after {first}: log-ratios differ in some bit"
            if first in results:  # (the same variant set again later, after the others came and went: the same decode)
                assert np.array_equal(before[0], results[first][0]) and bits_equal(before[1], results[first][1])
            results[first] = before
            setters[first](None)
            assert not any(held().values())
        # the three are three decodes, none of them the plain one -- what was compared above is the variant's own result
        outs = [plain] + [results[name] for name in SPELLING]
        for a, b in itertools.combinations(range(4), 2):
            assert not (np.array_equal(outs[a][0], outs[b][0]) and np.array_equal(outs[a][2], outs[b][2]) and bits_equal(outs[a][1], outs[b][1]))
        back = eng.decode_batch(c["synd"])
        assert np.array_equal(back[0], plain[0]) and np.array_equal(back[2], plain[2]) and bits_equal(back[1], plain[1]), "all off: the plain decode again"
    finally:
        eng.close()
