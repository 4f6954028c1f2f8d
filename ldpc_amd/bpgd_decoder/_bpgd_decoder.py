"""BP with guided decimation (BPGD): rounds of ``round_iters`` min-sum iterations on the flooding schedule; a round that ends without a
solution freezes the most reliable bit -- the largest ``|posterior|``, the smallest index among equal ones -- at ``+-freeze_llr`` of its
current sign, keeps every message, and the next round goes on.  All rounds of a batch are decoded in ONE call of the library
(``ldpc_hip_bp_set_decimation``) on the lane = edge kernels, nothing leaving the chip between rounds; the results are those of the NumPy
restatement tests/bpgd_util.py, bit for bit.  Codes beyond the lane = edge kernels are refused (``BpgdDecoder.route``: ``"unavailable"``):
the lane = node route for them and a per-pass route are not built yet."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

from ldpc_amd.bp_decoder._bp_decoder import BpDecoder

# bp_edge8's rungs (rounds of 64 slots) per column weight: LDPC_EDGE8_LADDER, ldpc_amd/csrc/bp_edge_kernel.h
_EDGE8_RUNGS = {3: (2, 3, 4, 5, 6, 7, 8, 9, 10, 12), 4: (2, 3, 4, 5, 6, 7, 8, 9)}


def _count(name, value, least):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
        raise ValueError(f"{name} must be an integer >= {least}, not {value!r}.")
    return int(value)


def decimation_schedule(n, *, round_iters=5, max_rounds=None, freeze_llr=25.0):
    """-> ``(round_iters, max_rounds, freeze_llr)`` checked: ``round_iters >= 1``; ``max_rounds >= 1`` or ``None`` for ``n`` (every bit can be
    frozen once); their product within int32 (it bounds the iteration count); ``freeze_llr`` positive, finite or ``inf``."""
    round_iters = _count("round_iters", round_iters, 1)
    max_rounds = max(1, int(n)) if max_rounds is None else _count("max_rounds", max_rounds, 1)
    if round_iters * max_rounds > 2 ** 31 - 1:
        raise ValueError(f"round_iters {round_iters} x max_rounds {max_rounds} does not fit the 32-bit iteration count.")
    try:
        c = float(freeze_llr)
    except (TypeError, ValueError):
        raise ValueError(f"freeze_llr must be a positive float (inf allowed), not {freeze_llr!r}.") from None
    if isinstance(freeze_llr, bool) or math.isnan(c) or c <= 0.0:
        raise ValueError(f"freeze_llr must be a positive float (inf allowed), not {freeze_llr!r}.")
    return round_iters, max_rounds, c


def lane_edge_route(pcm) -> str:
    """Which lane = edge kernel family takes the code under the default small-code kernel mode -- ``"bp_edge"`` (rows of at most 4 entries,
    columns of at most 2, 4 m <= 1024 slots), ``"bp_edge8"`` (rows <= 8, columns <= 4, 8 m slots within the family's ladder) or
    ``"unavailable"`` -- the rules of plan_edge / plan_edge8 (ldpc_amd/csrc/host_onchip.h), restated so that a decoder can say so without a GPU."""
    h = sp.csr_matrix(pcm)
    m, n = h.shape
    if m <= 0 or n <= 0 or h.nnz <= 0 or n > 65535 or h.nnz * 16 >= (1 << 22):
        return "unavailable"
    rows = int(np.diff(h.indptr).max())
    cols = np.bincount(h.indices, minlength=n)
    if int(cols.min()) < 1:  # a column without entries has no lane to write its outputs
        return "unavailable"
    cmax = int(cols.max())
    if rows <= 4 and cmax <= 2 and (4 * m + 63) // 64 <= 16:
        return "bp_edge"
    if rows <= 8 and cmax <= 4 and (8 * m + 63) // 64 <= _EDGE8_RUNGS[3 if cmax <= 3 else 4][-1]:
        return "bp_edge8"
    return "unavailable"


class BpgdDecoder(BpDecoder):
    """BP with guided decimation for binary linear codes, syndromes in, minimum-sum with the flooding schedule.  ``decode``, ``decode_batch``,
    ``converge``, ``iter`` (the iterations of all rounds a row ran), ``log_prob_ratios`` (of the last bit pass; a frozen bit's carries its
    ``+-freeze_llr``), ``update_channel_probs`` and the ``*_batch`` mirrors are ``BpDecoder``'s.  ``round_iters``, ``max_rounds`` and
    ``freeze_llr`` are read-only; ``decimation = dict(...)`` replaces them."""

    def __init__(self, pcm, error_rate=None, channel_probs=None, *, round_iters=5, max_rounds=None, freeze_llr=25.0, ms_scaling_factor=1.0, **kwargs):
        for key in kwargs:
            if key not in ("_device", "_backend"):
                raise ValueError(f"Unknown parameter '{key}' passed to the BpgdDecoder constructor.")
        if error_rate is None and channel_probs is None:
            raise ValueError("Please specify the error channel. Either: 1) error_rate: float or 2) channel_probs: list of floats of length equal to the block length of the code.")
        given = dict(kwargs)
        if error_rate is not None:
            given["error_rate"] = error_rate
        if channel_probs is not None:
            given["error_channel"] = channel_probs
        # (max_iter is not read while the decimation is on: the rounds take its place, and the setter below checks them)
        super().__init__(pcm, max_iter=1, bp_method="minimum_sum", ms_scaling_factor=ms_scaling_factor, schedule="parallel", input_vector_type="syndrome", **given)
        self.decimation = dict(round_iters=round_iters, max_rounds=max_rounds, freeze_llr=freeze_llr)

    @property
    def round_iters(self) -> int:
        return self._decimation[0]

    @property
    def max_rounds(self) -> int:
        return self._decimation[1]

    @property
    def freeze_llr(self) -> float:
        return self._decimation[2]

    @property
    def route(self) -> str:
        """``BpDecoder.decimation_route``: ``"bp_edge"``, ``"bp_edge8"`` or ``"unavailable"``."""
        return self.decimation_route
