#!/usr/bin/env python
"""Relay-BP (ldpc_hip_bp_set_relay): what the two routes cost, and whether the relay helps.

    python tools/bench_relay.py --speed      # (a) syndromes/s: the fused lane = edge route, the per-pass leg loop (small_mode 0), one memory decode of the same total iterations
    python tools/bench_relay.py --helps      # (b) BB144 x 12 rounds, p = 0.003: BP + OSD-0 as it is, relay + OSD-0, relay alone

(a) BB144 and the rotated surface code d = 21, min-sum, B = 65 536, p = 0.05, syndromes generated on the device, everything in HBM.  The
relay: a first leg of 30 iterations at strength 0.125, then 8 legs of 15 with strengths drawn from [-0.24, 0.66], stop at the first
solution.  One process, one engine per leg of the measurement, the legs ALTERNATING and every one run twice (``--passes``), each run =
``--warmup`` untimed decodes and ``--reps`` timed ones; one JSON line per leg and pass with the kernels its decode launched (the launch
log), and a summary line per code: the medians, the run-to-run spread of every leg (between its passes), the ratios, and the rule fixed
before anything was measured -- the fused route is the default for the lane = edge codes only if it beats the leg loop by more than the
spread of the two.
(b) the model of tools/bench_window.py (864 detectors x 2520 mechanisms; it runs the per-pass leg loop) through MonteCarloDemSimulation,
``--shots`` shots: min-sum 30 + OSD-0, the relay + OSD-0, the relay without OSD; rows left without a solution (+- sqrt), logical failures
(+- the binomial standard error), shots/s.  Lines go to stdout; ``--out FILE`` appends them to a file as well (profiles/relay_bp.jsonl).
Reads nothing but this repository.
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
RELAY = dict(gamma0=0.125, pre_iter=30, num_sets=8, set_max_iter=15, gamma_dist_interval=(-0.24, 0.66), stop_nconv=1, seed=0)


def emit(**line):
    text = json.dumps(line)
    print(text, flush=True)
    if _OUT:
        with open(_OUT, "a") as f:
            f.write(text + "\n")


def _engine(h, p, max_iter, relay=None, gamma=None, mode=None):
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.relay_decoder import relay_schedule
    h = h.tocsr()
    h.sort_indices()
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], np.full(h.shape[1], p), max_iter, 1, 0.625)
    if mode is not None:
        eng.set_small_code_kernel(mode)
    if gamma is not None:
        eng.set_memory(np.full(h.shape[1], gamma))
    if relay is not None:
        eng.set_relay(*relay_schedule(h.shape[1], **relay))
    return eng


def speed(batch, reps, warmup, passes):
    import torch
    from ldpc_amd import codes
    from ldpc_amd.engine import launch_log
    total = RELAY["pre_iter"] + RELAY["num_sets"] * RELAY["set_max_iter"]
    for name, h in (("bb144_p050", codes.bivariate_bicycle_hx()), ("surface_d21_p050", codes.rotated_surface_code_x(21))):
        legs = {"relay_fused": _engine(h, 0.05, 30, relay=RELAY), "relay_leg_loop": _engine(h, 0.05, 30, relay=RELAY, mode=0),
                "memory_same_total": _engine(h, 0.05, total, gamma=RELAY["gamma0"])}
        synd = legs["relay_fused"].gen_bsc_syndromes(12345, 0.05, 0, batch, device="cuda")
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
                        kernels = {k: v for k, v in sorted(log.items()) if k.startswith(("bp_", "relay_", "edge_relay"))}
                    else:
                        out = eng.decode_batch(synd, want_llr=False, out=out)
                    torch.cuda.synchronize()
                    if r >= warmup:
                        rates.append(batch / (time.perf_counter() - t0))
                medians[leg].append(float(np.median(rates)))
                emit(kind="relay_speed", config=name, leg=leg, run=ps, relay=None if leg == "memory_same_total" else {k: v for k, v in RELAY.items()},
                     max_iter=total if leg == "memory_same_total" else None, batch=batch, kernels=kernels,
                     syndromes_per_s=[round(x) for x in rates], median_syndromes_per_s=round(medians[leg][-1]),
                     converged=int(out[3].sum()), mean_iterations=round(float(out[2].double().mean()), 3))
        med = {k: float(np.median(v)) for k, v in medians.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in medians.items()}
        emit(kind="relay_speed_summary", config=name, batch=batch, median_syndromes_per_s={k: round(v) for k, v in med.items()},
             run_to_run_spread={k: round(v, 4) for k, v in spread.items()}, fused_over_leg_loop=round(med["relay_fused"] / med["relay_leg_loop"], 3),
             fused_beats_leg_loop_by_more_than_the_spread=bool(med["relay_fused"] / med["relay_leg_loop"] - 1 > spread["relay_fused"] + spread["relay_leg_loop"]),
             fused_over_memory_same_total=round(med["relay_fused"] / med["memory_same_total"], 3))
        for eng in legs.values():
            eng.close()


def helps(shots, batch, p):
    from ldpc_amd import codes
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from window_util import phenomenological_matrices
    model = phenomenological_matrices(codes.bivariate_bicycle_hx(), 12, p, p, logical=tuple(range(12)))
    for leg, relay, with_osd in (("bp30_osd0", None, True), ("relay_osd0", RELAY, True), ("relay_alone", RELAY, False)):
        sim = MonteCarloDemSimulation(model, target_run_count=shots, batch_size=batch, seed=5, max_iter=30, bp_method="ms", ms_scaling_factor=0.625,
                                      osd_method="osd0", relay=relay)
        eng = sim._get_engine()
        eng.simulate_b8(5, 0, min(batch, 4096), with_osd=with_osd)  # (untimed: allocations, tables)
        t0 = time.perf_counter()
        f = u = 0
        for shot0 in range(0, shots, batch):  # (the class's own loop, with the OSD switch it does not offer)
            df, du = eng.simulate_b8(5, shot0, min(batch, shots - shot0), chunk=min(batch, shots - shot0), with_osd=with_osd)
            f, u = f + df, u + du
        dt = time.perf_counter() - t0
        emit(kind="relay_helps", config=f"BB144 x 12 rounds, p = {p}, min-sum, alpha 0.625", leg=leg, relay=relay, shots=shots, unconverged=u,
             unconverged_counting_error=round(float(np.sqrt(u)), 1), logical_failures=f, logical_error_rate=f / shots,
             logical_error_rate_se=float(np.sqrt(max(f, 1) * (1 - f / shots)) / shots), shots_per_s=round(shots / dt))


def main():
    global _OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--speed", action="store_true")
    ap.add_argument("--helps", action="store_true")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--shots", type=int, default=1 << 20)
    ap.add_argument("--p", type=float, default=0.003)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _OUT = args.out
    if args.speed:
        speed(args.batch, args.reps, args.warmup, args.passes)
    if args.helps:
        helps(args.shots, args.batch, args.p)


if __name__ == "__main__":
    main()
