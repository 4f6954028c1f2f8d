"""Row-prior fixtures (tests/golden/row_priors/row_priors_*.npz, written by tests/golden/make_golden_row_priors.py): what the reference
returns for the loop ``d.update_channel_probs(P[b]); d.decode(S[b])``.  They live in their own directory: the loader of the shared-prior
fixtures (tests/golden_util.py) lists every ``tests/golden/*.npz`` for the parity tests, and these files have rows of priors, not one.

The builders below are shared by the generator and the tests, so that a fixture stores only what cannot be rebuilt: the probabilities as
an index into a short table of levels (the special values 0, 1, 0.5, 1e-300, 1 - 2^-53 among them), the syndromes, the reference's
decisions / flags / iteration counts, its log-ratios in full for the first rows and as a per-row checksum for all of them."""
from __future__ import annotations

import glob
import os
import zlib

import numpy as np
import scipy.sparse as sp

ROW_PRIORS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_priors")
SPECIAL = (0.0, 1.0, 0.5, 1e-300, 1.0 - 2.0 ** -53)  # priors +inf, -inf, +0.0, ~690.8, ~-36.7 (bp.hpp:150-151)


def case_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROW_PRIORS_DIR, "row_priors_*.npz")))


def llr_digest(llr: np.ndarray) -> np.ndarray:
    """(B,) uint32: checksum of every row's bit patterns, any NaN counted as one NaN (``oracle.bits_equal``'s rule)."""
    a = np.ascontiguousarray(llr, np.float64).copy()
    a[np.isnan(a)] = np.nan
    return np.array([zlib.crc32(row.tobytes()) for row in a], np.uint32)


def draw_levels(rng, shape, levels, special_rows=()):
    """Indices into ``levels`` (the ordinary ones: beyond ``len(SPECIAL)``), different in every row; the rows named in ``special_rows``
    get the special values sprinkled over a third of their bits."""
    k0 = len(SPECIAL)
    idx = rng.integers(k0, len(levels), size=shape).astype(np.uint8)
    for r in special_rows:
        where = rng.random(shape[1]) < 1.0 / 3.0
        idx[r, where] = rng.integers(0, k0, size=int(where.sum())).astype(np.uint8)
    assert len({row.tobytes() for row in idx}) == shape[0], "two rows drew the same priors"
    return idx


def levels_around(p, count=11, spread=4.0):
    """The special values, then ``count`` ordinary probabilities geometrically spaced from p / spread to p * spread."""
    return np.array(SPECIAL + tuple(p * spread ** (2.0 * k / (count - 1) - 1.0) for k in range(count)), np.float64)


def syndromes_of(h, probs, rng):
    """s = H e with e[b][j] ~ Bernoulli(P[b][j]): every row's errors drawn at its own rates."""
    e = (rng.random(probs.shape) < probs).astype(np.uint8)
    return np.ascontiguousarray((sp.csr_matrix(h, dtype=np.int64) @ e.T.astype(np.int64)).T % 2, np.uint8)


def load_case(name: str) -> dict:
    z = np.load(os.path.join(ROW_PRIORS_DIR, name + ".npz"), allow_pickle=False)
    m, n = int(z["m"]), int(z["n"])
    ci, rp = z["col_idx"], z["row_ptr"]
    h = sp.csr_matrix((np.ones(len(ci), np.uint8), ci, rp), shape=(m, n), dtype=np.uint8)
    return dict(
        name=name, h=h, m=m, n=n, probs=np.ascontiguousarray(z["levels"][z["p_idx"]], np.float64), own_p=float(z["own_p"]),
        syndromes=np.ascontiguousarray(z["syndromes"], np.uint8), max_iter=int(z["max_iter"]),
        bp_method=("product_sum", "minimum_sum")[int(z["bp_method"])], ms_scaling_factor=float(z["ms_scaling_factor"]),
        osd=bool(z["osd"]), decoding=np.unpackbits(z["decoding"], axis=1, count=n), converge=z["converge"].astype(bool),
        iterations=z["iterations"].astype(np.int32), llr=z["llr"], llr_crc=z["llr_crc"].astype(np.uint32), note=str(z["note"]))


def ran_bp(case) -> np.ndarray:
    """Rows that ran BP: an all-zero syndrome takes the reference's shortcut (pyx:679-681) -- zeros, converge, nothing else touched."""
    return case["syndromes"].any(axis=1)
