"""BP with guided decimation (BPGD): rounds of ``round_iters`` min-sum iterations on the flooding schedule; a round that ends without a
solution freezes the most reliable bit -- the largest ``|posterior|``, the smallest index among equal ones -- at ``+-freeze_llr`` of its
current sign, keeps every message, and the next round goes on.  All rounds of a batch are decoded in ONE call of the library
(``ldpc_hip_bp_set_decimation``), nothing leaving the chip between rounds; the results are those of the NumPy restatement
tests/bpgd_util.py, bit for bit.  By default on the lane = edge kernels only: codes beyond them are refused (``BpgdDecoder.route``:
``"unavailable"``).  ``lane_node=True`` opts in to the lane = node kernel for those codes (rows of at most 16, columns of at most 8 entries, a
syndrome's state within LDS: ``lane_node_takes``); a per-pass route is not built."""
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


_WAVE_RUNGS = ((4, 2), (4, 4), (6, 3), (8, 4), (8, 8), (16, 8))  # bp_wave_gd_kernel's instantiations (rows, columns)
# WAVE_GD_LDS_STATIC (ldpc_amd/csrc/bp_wave_gd_kernel.h): what plan_wave_gd leaves free of a workgroup's 160 KiB for the kernel's static LDS
# -- 224 bytes in the team forms: two flags, the team's syndrome number, sixteen winners of 8 + 4 bytes, the clock stamps
_WAVE_GD_LDS_STATIC = 256


def lane_node_takes(pcm) -> bool:
    """Whether the lane = node decimation kernel takes the code under the default small-code kernel mode -- the rules of plan_wave_gd
    (ldpc_amd/csrc/host_onchip.h) restated without a GPU: rows of at most 16 entries and columns of at most 8; 16-bit positions; padding every
    row to the rung's weight costs at most twice the entries plus 1024; the shared tables and one syndrome's private region (messages,
    posteriors, the hard-decision word and the two decimation masks, the syndrome bytes) within 160 KiB - 256 of LDS (the 256: the kernel's
    static LDS).  It says nothing about the lane = edge families, which are asked first (``lane_edge_route``).  The DEFAULT mode only: an engine
    whose small-code kernel mode is 1, 3, 4 or 5 waives the padding rule, so the decoder classes -- which expose no kernel mode and refuse
    before a handle exists what this function and ``lane_edge_route`` both turn down -- refuse such a code although a forced engine decodes it."""
    h = sp.csr_matrix(pcm)
    m, n = h.shape
    if m <= 0 or n <= 0 or h.nnz <= 0 or h.nnz * 16 >= (1 << 22):
        return False
    rows = int(np.diff(h.indptr).max())
    cmax = int(np.bincount(h.indices, minlength=n).max())
    rung = next(((r, c) for r, c in _WAVE_RUNGS if rows <= r and cmax <= c), None)
    if rung is None:
        return False
    dr, dc = rung
    mp, np_ = (m + 63) // 64 * 64, (n + 63) // 64 * 64
    rm = dr * mp
    if rm + 2 >= 65536 or np_ + 1 >= 65536 or rm > 2 * h.nnz + 1024:
        return False
    up16 = lambda b: (b + 15) & ~15  # noqa: E731
    shared = up16(rm * 2 + dc * np_ * 2 + mp)
    private = up16((rm + 2) * 8 + np_ * 8 + 3 * (np_ // 64 + 1) * 8 + mp)
    return shared + private <= 160 * 1024 - _WAVE_GD_LDS_STATIC


class BpgdDecoder(BpDecoder):
    """BP with guided decimation for binary linear codes, syndromes in, minimum-sum with the flooding schedule.  ``decode``, ``decode_batch``,
    ``converge``, ``iter`` (the iterations of all rounds a row ran), ``log_prob_ratios`` (of the last bit pass; a frozen bit's carries its
    ``+-freeze_llr``), ``update_channel_probs`` and the ``*_batch`` mirrors are ``BpDecoder``'s.  ``round_iters``, ``max_rounds`` and
    ``freeze_llr`` are read-only; ``decimation = dict(...)`` replaces them.  ``lane_node=True`` sets ``decimation_lane_node``: a code beyond
    the lane = edge kernels goes to the lane = node kernel instead of being refused."""

    def __init__(self, pcm, error_rate=None, channel_probs=None, *, round_iters=5, max_rounds=None, freeze_llr=25.0, ms_scaling_factor=1.0, lane_node=False, **kwargs):
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
        self.decimation_lane_node = lane_node

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
        """``BpDecoder.decimation_route``: ``"bp_edge"``, ``"bp_edge8"``, with ``lane_node`` also ``"bp_wave"`` / ``"bp_wave_team"``, or ``"unavailable"``."""
        return self.decimation_route
