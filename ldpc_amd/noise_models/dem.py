"""Shots of a detector error model: independent error mechanisms with their own probabilities, detection events and observables.

``generate_dem_batch`` is the NumPy twin of the device sampler (``HipBpEngine.sample_b8`` / ``ldpc_hip_bp_sample_b8``) and its
specification -- the reference has no sampler (its users bring ``stim``'s ``compile_sampler``), so the contract is this function and the
device reproduces it bit for bit:

* thresholds ``T[j] = prng.bernoulli_thresholds(p)[j]`` = ``min(max(ceil(p[j] * 2**53), 0), 2**53)``: ``p = 0`` never fires, ``p = 1`` always;
* errors ``e[b][j] = (sm64(seed, (shot0 + b) * n + j) >> 11) < T[j]``, the index taken in uint64 -- the convention of ``generate_bsc_batch``,
  whose errors these are when all ``p[j]`` are equal; any shard of a run can be regenerated from ``(seed, shot0)`` alone;
* detection events ``H e mod 2`` and true observables ``L e mod 2``, bit-packed in stim's "b8" layout (bit i of a shot is bit ``i % 8`` of
  byte ``i // 8``, every shot starts on a byte, padding bits are 0); the errors come in the same packing.

Host only.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from ldpc_amd.prng import bernoulli_thresholds, sm64


def check_dem_probabilities(priors, n: int) -> np.ndarray:
    """``priors`` as a float64 vector of length ``n``; ``ValueError`` for another length, a value outside [0, 1] or NaN."""
    p = np.asarray(priors, dtype=np.float64)
    if p.shape != (int(n),):
        raise ValueError(f"Probabilities vector must have length equal to the number of error mechanisms ({n}), not shape {p.shape}")
    bad = int(np.count_nonzero(~((p >= 0.0) & (p <= 1.0))))
    if bad:
        raise ValueError(f"Probabilities must lie in [0, 1]: {bad} values are outside it or NaN")
    return np.ascontiguousarray(p)


def pack_b8(bits: np.ndarray) -> np.ndarray:
    """``(B, bits)`` 0/1 -> ``(B, ceil(bits / 8))`` uint8 in the b8 layout."""
    bits = np.asarray(bits, dtype=np.uint8)
    if bits.shape[1] == 0:
        return np.zeros((bits.shape[0], 0), np.uint8)
    return np.packbits(bits, axis=1, bitorder="little")


def generate_dem_batch(check, observables, priors, seed: int, shot0: int, shots: int):
    """``(errors, dets, obs)`` of shots ``shot0 .. shot0 + shots - 1`` of stream ``seed``, each b8-packed:
    ``(shots, ceil(n/8))``, ``(shots, ceil(m/8))``, ``(shots, ceil(k/8))`` for an ``m x n`` check matrix and ``k x n`` observables."""
    h = sp.csr_matrix(check, dtype=np.int64)
    m, n = h.shape
    if observables is None:
        obs_m = sp.csr_matrix((0, n), dtype=np.int64)
    else:
        obs_m = sp.csr_matrix(observables, dtype=np.int64)
        if obs_m.shape[1] != n:
            raise ValueError(f"observables must have {n} columns")
    p = check_dem_probabilities(priors, n)
    if shot0 < 0 or shots < 0:
        raise ValueError("shot0 and shots must not be negative")
    thr = bernoulli_thresholds(p)
    with np.errstate(over="ignore"):
        idx = (np.arange(shots, dtype=np.uint64) + np.uint64(shot0))[:, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :]
    e = ((sm64(seed, idx) >> np.uint64(11)) < thr[None, :]).astype(np.uint8)
    e64 = e.astype(np.int64)
    dets = np.asarray((h @ e64.T).T % 2, dtype=np.uint8).reshape(shots, m)
    obs = np.asarray((obs_m @ e64.T).T % 2, dtype=np.uint8).reshape(shots, obs_m.shape[0])
    return pack_b8(e), pack_b8(dets), pack_b8(obs)
