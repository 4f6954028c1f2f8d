"""Relay-BP: a first memory min-sum leg with one strength everywhere, then ``num_sets`` legs with per-bit strengths drawn once, each started
from the posteriors the leg before it ended with; the lightest of the first ``stop_nconv`` solutions is the result.  The legs of a batch are
decoded in ONE call of the library (``ldpc_hip_bp_set_relay``): on the lane = edge relay kernels where the code fits them, on the lane = node
kernel ``bp_wave_relay_kernel`` where the small-code kernel mode asks for it, else as a loop of per-pass memory decodes on the device -- the
results are the same bits (tests/relay_bp_util.py is the contract); ``RelayBpDecoder.route`` names the route taken."""
from __future__ import annotations

import numpy as np

from ldpc_amd.bp_decoder._bp_decoder import BpDecoder


def _count(name, value, least):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
        raise ValueError(f"{name} must be an integer >= {least}, not {value!r}.")
    return int(value)


def relay_schedule(n, *, gamma0=0.125, pre_iter=80, num_sets=60, set_max_iter=60, gamma_dist_interval=(-0.24, 0.66), stop_nconv=1,
                   strengths=None, seed=0):
    """-> ``(strengths (legs, n) float64, leg_iters (legs,) int32, stop_after)``.  Leg 0 has strength ``gamma0`` everywhere and ``pre_iter``
    iterations; legs 1 .. ``num_sets`` have ``set_max_iter`` iterations each and strengths drawn once with
    ``np.random.default_rng(seed).uniform(*gamma_dist_interval, (num_sets, n))``.  An explicit ``strengths`` array of shape ``(legs, n)``
    overrides the drawing (leg 0 included; ``legs`` = ``num_sets + 1`` is then read off its shape).  Every strength must be finite and in
    ``[-1, 1)``."""
    pre_iter = _count("pre_iter", pre_iter, 1)
    stop_nconv = _count("stop_nconv", stop_nconv, 1)
    if strengths is not None:
        g = np.array(strengths, dtype=np.float64)
        if g.ndim != 2 or g.shape[1] != n or g.shape[0] < 1:
            raise ValueError(f"strengths must have shape (legs, {n}), not {g.shape}.")
        num_sets = g.shape[0] - 1
    else:
        num_sets = _count("num_sets", num_sets, 0)
        seed = _count("seed", seed, 0)
        try:
            lo, hi = (float(x) for x in gamma_dist_interval)
        except (TypeError, ValueError):
            raise ValueError(f"gamma_dist_interval must be a pair of floats, not {gamma_dist_interval!r}.") from None
        if not (np.isfinite(lo) and np.isfinite(hi) and -1.0 <= lo <= hi < 1.0):
            raise ValueError(f"gamma_dist_interval must satisfy -1 <= low <= high < 1, not {gamma_dist_interval!r}.")
        g = np.empty((num_sets + 1, n), np.float64)
        g[0] = float(gamma0)
        g[1:] = np.random.default_rng(seed).uniform(lo, hi, (num_sets, n))
    if num_sets:
        set_max_iter = _count("set_max_iter", set_max_iter, 1)
    if not (np.isfinite(g).all() and (g >= -1.0).all() and (g < 1.0).all()):
        raise ValueError("relay strengths (gamma0 included): every strength must be finite and in [-1, 1).")
    leg_iters = np.full(num_sets + 1, set_max_iter if num_sets else pre_iter, np.int32)
    leg_iters[0] = pre_iter
    return g, leg_iters, stop_nconv


class RelayBpDecoder(BpDecoder):
    """Relay-BP decoder for binary linear codes, syndromes in, minimum-sum with the flooding schedule.  ``decode``, ``decode_batch``,
    ``converge``, ``iter`` (the iterations of all legs a row ran), ``log_prob_ratios`` (of the chosen solution; of the last leg where none was
    found), ``update_channel_probs`` and the ``*_batch`` mirrors are ``BpDecoder``'s.  ``strengths`` and ``leg_iters`` are read-only."""

    def __init__(self, pcm, error_rate=None, channel_probs=None, *, gamma0=0.125, pre_iter=80, num_sets=60, set_max_iter=60,
                 gamma_dist_interval=(-0.24, 0.66), stop_nconv=1, ms_scaling_factor=1.0, strengths=None, seed=0, **kwargs):
        for key in kwargs:
            if key not in ("_device", "_backend"):
                raise ValueError(f"Unknown parameter '{key}' passed to the RelayBpDecoder constructor.")
        if error_rate is None and channel_probs is None:
            raise ValueError("Please specify the error channel. Either: 1) error_rate: float or 2) channel_probs: list of floats of length equal to the block length of the code.")
        given = dict(kwargs)
        if error_rate is not None:
            given["error_rate"] = error_rate
        if channel_probs is not None:
            given["error_channel"] = channel_probs
        super().__init__(pcm, max_iter=int(pre_iter) if isinstance(pre_iter, (int, np.integer)) and not isinstance(pre_iter, bool) and pre_iter > 0 else 1,
                         bp_method="minimum_sum", ms_scaling_factor=ms_scaling_factor, schedule="parallel", input_vector_type="syndrome", **given)
        self.relay = dict(gamma0=gamma0, pre_iter=pre_iter, num_sets=num_sets, set_max_iter=set_max_iter, gamma_dist_interval=gamma_dist_interval,
                          stop_nconv=stop_nconv, strengths=strengths, seed=seed)

    @property
    def strengths(self) -> np.ndarray:
        return self._relay[0].copy()

    @property
    def leg_iters(self) -> np.ndarray:
        return self._relay[1].copy()

    @property
    def stop_nconv(self) -> int:
        return self._relay[2]

    @property
    def route(self) -> str:
        """``BpDecoder.relay_route``: ``"per_pass"``, ``"bp_edge"``, ``"bp_edge8"``, ``"bp_wave"`` or ``"bp_wave_team"``."""
        return self.relay_route
