#!/usr/bin/env python3
"""What per-row channel probabilities (decode_batch(..., channel_probs=P)) cost against the SAME build's shared-prior decode on the SAME
forced kernel, timed in one process, the two interleaved call by call:

  * the headline code ((3,6)-regular, n = 10 000, product-sum 50 at p = 0.05), B = 4 096, per-pass kernels forced (set_handoff above
    the tile count: the path a row-prior decode takes), plain against row priors;
  * BB [[144,12,12]] hx, product-sum 50 at p = 0.05, B = 8 192, slot kernel forced (set_small_code_kernel 2), plain against row priors.

Every row of P is the handle's own probability, so both sides do the same arithmetic and must return the same bits (checked); the
difference is the priors' traffic: a conversion pass and one 512-byte segment per bit per bit pass (per-pass kernels), a strided read
per slot refill (slot kernel).  Also printed: the box's copy-probe rate from the same run.  No threshold: numbers for NOTES.md.
Run on an MI355X:   python tools/bench_row_priors.py [--reps 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldpc_amd import codes  # noqa: E402
from ldpc_amd.engine import HipBpEngine  # noqa: E402


def pair(name, h, p, max_iter, batch, setup, reps):
    h = sp.csr_matrix(h)
    h.sort_indices()
    m, n = h.shape
    eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, p), max_iter, 0, 1.0)
    setup(eng)
    s = eng.gen_bsc_syndromes(7, p, shot0=0, shots=batch, device="cuda:0")
    probs = torch.full((batch, n), p, dtype=torch.float64, device="cuda:0")
    outs = {"plain": eng.decode_batch(s), "row_priors": None}
    outs["plain"] = [o.clone() for o in outs["plain"]]
    outs["row_priors"] = [o.clone() for o in eng.decode_batch(s, channel_probs=probs)]
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b))
               for a, b in zip(outs["plain"], outs["row_priors"]))
    wall, kern = {"plain": [], "row_priors": []}, {"plain": [], "row_priors": []}
    for _ in range(reps):
        for key, kw in (("plain", {}), ("row_priors", {"channel_probs": probs})):  # interleaved: both see the same clocks and neighbours
            t0 = time.perf_counter()
            eng.decode_batch(s, asynchronous=True, **kw)
            torch.cuda.synchronize()
            wall[key].append((time.perf_counter() - t0) * 1e3)
            kern[key].append(eng.last_kernel_ms())
    tiles = (batch + 63) // 64
    probe_ms, probe_rate = eng.copy_probe(min(tiles, 64))
    med = lambda v: float(np.median(v))  # noqa: E731
    res = {"config": name, "m": m, "n": n, "nnz": int(h.nnz), "batch": batch, "max_iter": max_iter, "p": p, "reps": reps,
           "mean_iterations": round(float(outs["plain"][2].float().mean()), 2), "identical": same,
           "wall_ms": {k: round(med(v), 4) for k, v in wall.items()}, "kernel_ms": {k: round(med(v), 4) for k, v in kern.items()},
           "ratio_plain_over_row_priors_wall": round(med(wall["plain"]) / med(wall["row_priors"]), 4),
           "ratio_plain_over_row_priors_kernel": round(med(kern["plain"]) / med(kern["row_priors"]), 4) if med(kern["row_priors"]) > 0 else None,
           "copy_probe_GBps": round(probe_rate, 1)}
    print(json.dumps(res), flush=True)
    eng.close()
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    ok = pair("headline (3,6) n=10000 ps50, per-pass forced", codes.regular_ldpc_code(10000, 3, 6, seed=1), 0.05, 50, 4096,
              lambda e: (e.set_handoff(1 << 20), e.set_repack(0)), args.reps)
    ok &= pair("BB144 hx ps50, slot kernel forced", codes.bivariate_bicycle_hx(), 0.05, 50, 8192, lambda e: e.set_small_code_kernel(2), args.reps)
    print("IDENTICAL" if ok else "MISMATCH")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
