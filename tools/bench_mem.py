#!/usr/bin/env python
"""Memory min-sum BP (ldpc_hip_bp_set_memory): what it costs, and whether it helps.

    python tools/bench_mem.py --speed      # (a) syndromes/s: plain decode, memory decode (gamma = 0.35), memory on the per-pass kernels (small_mode 0)
    python tools/bench_mem.py --helps      # (b) BB144 x 12 rounds, p = 0.003, min-sum 30 + OSD-0: unconverged rows, logical failures, shots/s per gamma

(a) BB144 and the rotated surface code d = 21, min-sum 30, B = 65 536, p = 0.05, syndromes generated on the device, everything in HBM.  One
process, one engine per leg, the legs ALTERNATING (plain, memory, per-pass memory, plain, ...) and every leg run twice (``--passes``), each
run = ``--warmup`` untimed decodes and ``--reps`` timed ones; one JSON line per leg and pass with the BP kernels its decode launched (the
launch log), and a summary line per code: the medians, the run-to-run spread of every leg (between its passes) and the two ratios.
(b) the model of tools/bench_window.py (864 detectors x 2520 mechanisms) through MonteCarloDemSimulation, 2^20 shots: plain, then scalar
gamma in {0.125, 0.35, 0.6}; logical failures with their binomial standard error.  Lines go to stdout; ``--out FILE`` appends them to a
file as well (profiles/mem_bp.jsonl).  Reads nothing but this repository.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

_OUT = None


def emit(**line):
    text = json.dumps(line)
    print(text, flush=True)
    if _OUT:
        with open(_OUT, "a") as f:
            f.write(text + "\n")


def _engine(h, p, max_iter, gamma=None, mode=None):
    from ldpc_amd.engine import HipBpEngine
    h = h.tocsr()
    h.sort_indices()
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], np.full(h.shape[1], p), max_iter, 1, 0.625)
    if mode is not None:
        eng.set_small_code_kernel(mode)
    if gamma is not None:
        eng.set_memory(np.full(h.shape[1], gamma))
    return eng


def speed(batch, reps, warmup, passes, gamma):
    import torch
    from ldpc_amd import codes
    from ldpc_amd.engine import launch_log
    for name, h in (("bb144_ms30_p050", codes.bivariate_bicycle_hx()), ("surface_d21_ms30_p050", codes.rotated_surface_code_x(21))):
        legs = {"plain": _engine(h, 0.05, 30), "memory": _engine(h, 0.05, 30, gamma), "memory_per_pass": _engine(h, 0.05, 30, gamma, mode=0)}
        synd = legs["plain"].gen_bsc_syndromes(12345, 0.05, 0, batch, device="cuda")
        medians = {k: [] for k in legs}
        for ps in range(passes):
            for leg, eng in legs.items():  # alternating: every pass visits every leg
                out, rates, kernels = None, [], None
                for r in range(reps + warmup):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if r == 0:
                        with launch_log() as log:
                            out = eng.decode_batch(synd, want_llr=False, out=out)
                            torch.cuda.synchronize()
                        kernels = {k: v for k, v in sorted(log.items()) if k.startswith("bp_")}
                    else:
                        out = eng.decode_batch(synd, want_llr=False, out=out)
                    torch.cuda.synchronize()
                    if r >= warmup:
                        rates.append(batch / (time.perf_counter() - t0))
                medians[leg].append(float(np.median(rates)))
                emit(kind="mem_speed", config=name, leg=leg, run=ps, gamma=None if leg == "plain" else gamma, batch=batch, bp_kernels=kernels,
                     syndromes_per_s=[round(x) for x in rates], median_syndromes_per_s=round(medians[leg][-1]), kernel_ms=round(eng.last_kernel_ms(), 3),
                     converged=int(out[3].sum()), mean_iterations=round(float(out[2].double().mean()), 3))
        med = {k: float(np.median(v)) for k, v in medians.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in medians.items()}
        emit(kind="mem_speed_summary", config=name, batch=batch, median_syndromes_per_s={k: round(v) for k, v in med.items()},
             run_to_run_spread={k: round(v, 4) for k, v in spread.items()}, memory_over_per_pass=round(med["memory"] / med["memory_per_pass"], 3),
             edge_route_beats_per_pass_by_more_than_the_spread=bool(med["memory"] / med["memory_per_pass"] - 1 > spread["memory"] + spread["memory_per_pass"]),
             memory_over_plain=round(med["memory"] / med["plain"], 3))
        for eng in legs.values():
            eng.close()


def helps(shots, batch, gammas, p):
    from ldpc_amd import codes
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from window_util import phenomenological_matrices
    model = phenomenological_matrices(codes.bivariate_bicycle_hx(), 12, p, p, logical=tuple(range(12)))
    for gamma in [None] + list(gammas):
        sim = MonteCarloDemSimulation(model, target_run_count=shots, batch_size=batch, seed=5, max_iter=30, bp_method="ms", ms_scaling_factor=0.625,
                                      osd_method="osd0", memory_strength=gamma)
        sim._get_engine().simulate_b8(5, 0, min(batch, 4096), with_osd=True)  # (untimed: allocations, tables)
        t0 = time.perf_counter()
        res = sim.run()
        dt = time.perf_counter() - t0
        n, f, u = res["run_count"], res["fail_count"], res["bp_unconverged_count"]
        emit(kind="mem_helps", config=f"BB144 x 12 rounds, p = {p}, min-sum 30 + OSD-0", gamma=gamma, shots=n, bp_unconverged=u,
             bp_unconverged_counting_error=round(float(np.sqrt(u)), 1), logical_failures=f, logical_error_rate=f / n,
             logical_error_rate_se=float(np.sqrt(max(f, 1) * (1 - f / n)) / n), shots_per_s=round(n / dt))


def main():
    global _OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--speed", action="store_true")
    ap.add_argument("--helps", action="store_true")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--gamma", type=float, default=0.35)
    ap.add_argument("--shots", type=int, default=1 << 20)
    ap.add_argument("--gammas", default="0.125,0.35,0.6")
    ap.add_argument("--p", type=float, default=0.003)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _OUT = args.out
    if args.speed:
        speed(args.batch, args.reps, args.warmup, args.passes, args.gamma)
    if args.helps:
        helps(args.shots, args.batch, [float(x) for x in args.gammas.split(",")], args.p)


if __name__ == "__main__":
    main()
