#!/usr/bin/env python
"""BP with guided decimation on the lane = node kernel (ldpc_hip_bp_set_decimation_lane_node): what it costs, how many
rows it solves beyond the lane = edge codes, and the logical error rate on a detector error model.

    python tools/bench_bpgd_dem.py --speed                  # (a) device-resident, B = 65 536: HGP [[400,16]] and [[1600,64]] at p = 0.02, BB288 at p = 0.05
    python tools/bench_bpgd_dem.py --dem                    # (b) BB144 x 12 rounds, p = 0.003, 2^20 shots through MonteCarloDemSimulation's engine
    python tools/bench_bpgd_dem.py --bench LIB              # (c) bench.py --gpus 1 --steps 5 --warmup 2, this build alternating with the build at LIB

Min-sum, alpha 0.625, T = 5, C = 25.
(a) legs: plain min-sum 30; plain min-sum with BPGD's iteration budget (5 R); the relay of section 7d (30 iterations at strength 0.125, then 8
legs of 15 drawn from [-0.24, 0.66], stop at the first solution); BPGD with R = 16 and R = 64 (lane = node switch on) -- ALTERNATING, every
leg ``--passes`` times, each run = ``--warmup`` untimed and ``--reps`` timed decodes of syndromes generated on the device; one JSON line per
leg and pass with the launch log of an untimed decode of its own, rows solved and mean iterations; a summary per code.
(b) the model of tools/bench_relay_wave.py --dem: BPGD + OSD-0 (R = 16 and R = 64: R = n would be 12 600 iterations for an unsolved row), min-sum
30 + OSD-0, relay + OSD-0; shots/s, rows left for OSD (+- sqrt), logical failures (+- the binomial standard error); every leg ``--passes`` times.
(c) tools/bench_bpgd.py's headline leg.
Nothing is gated on these figures.  Lines go to stdout; ``--out FILE`` appends them to a file as well (profiles/bpgd_wave.jsonl).  Reads nothing
but this repository (and LIB).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_bpgd  # noqa: E402  (emit, the relay's schedule, the headline leg)

emit, RELAY, ROUND_ITERS, FREEZE = bench_bpgd.emit, bench_bpgd.RELAY, bench_bpgd.ROUND_ITERS, bench_bpgd.FREEZE
ROUNDS = (16, 64)


def _engine(h, p, max_iter, relay=None, decimation=None):
    eng = bench_bpgd._engine(sp.csr_matrix(h), p, max_iter, relay=relay)
    if decimation is not None:
        eng.set_decimation_lane_node(True)
        eng.set_decimation(*decimation)
    return eng


def _spread(values):
    med = {k: float(np.median(v)) for k, v in values.items()}
    return med, {k: (max(v) - min(v)) / med[k] for k, v in values.items()}


def speed(batch, reps, warmup, passes):
    import torch
    from ldpc_amd import codes
    from ldpc_amd.codes.synthetic import bivariate_bicycle_hx
    from ldpc_amd.engine import launch_log
    hgp = lambda n: codes.hypergraph_product_hx(codes.regular_ldpc_code(n, 3, 4, seed=5))  # noqa: E731
    bb288 = bivariate_bicycle_hx(12, 12, (("x", 3), ("y", 2), ("y", 7)), (("y", 3), ("x", 1), ("x", 2)))
    for name, h, p in (("hgp400_p020", hgp(16), 0.02), ("hgp1600_p020", hgp(32), 0.02), ("bb288_p050", bb288, 0.05)):
        settings = {"plain_30": dict(max_iter=30), "relay": dict(max_iter=30, relay=RELAY)}
        for r in ROUNDS:
            settings[f"plain_budget_{ROUND_ITERS * r}"] = dict(max_iter=ROUND_ITERS * r)
            settings[f"bpgd_R_{r}"] = dict(max_iter=30, decimation=(ROUND_ITERS, r, FREEZE))
        legs = {k: _engine(h, p, **kw) for k, kw in settings.items()}
        routes = {k: legs[k].decimation_route(batch) for k in legs if k.startswith("bpgd")}
        synd = legs["plain_30"].gen_bsc_syndromes(12345, p, 0, batch, device="cuda")
        medians, solved, mean_it = {k: [] for k in legs}, {}, {}
        for ps in range(passes):
            for leg, eng in legs.items():  # alternating: every pass visits every leg
                rates = []
                with launch_log() as log:  # (an untimed decode of its own carries the log hook)
                    out = eng.decode_batch(synd, want_llr=False)
                    torch.cuda.synchronize()
                kernels = {k: v for k, v in sorted(log.items()) if k.startswith(("bp_", "relay_", "wave_"))}
                for r in range(reps + warmup):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = eng.decode_batch(synd, want_llr=False, out=out)
                    torch.cuda.synchronize()
                    if r >= warmup:
                        rates.append(batch / (time.perf_counter() - t0))
                medians[leg].append(float(np.median(rates)))
                solved[leg], mean_it[leg] = int(out[3].sum()), round(float(out[2].double().mean()), 3)
                kw = settings[leg]
                emit(kind="bpgd_wave_speed", config=name, leg=leg, run=ps, max_iter=None if len(kw) > 1 else kw["max_iter"], relay=kw.get("relay"),
                     decimation=kw.get("decimation"), route=routes.get(leg), batch=batch, p=p, kernels=kernels, syndromes_per_s=[round(x) for x in rates],
                     median_syndromes_per_s=round(medians[leg][-1]), converged=solved[leg], mean_iterations=mean_it[leg])
        med, spread = _spread(medians)
        emit(kind="bpgd_wave_speed_summary", config=name, batch=batch, p=p, routes=routes, median_syndromes_per_s={k: round(v) for k, v in med.items()},
             run_to_run_spread={k: round(v, 4) for k, v in spread.items()}, rows_solved=solved, mean_iterations=mean_it)
        for eng in legs.values():
            eng.close()


def dem(shots, batch, p, passes):
    from ldpc_amd import codes
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from window_util import phenomenological_matrices
    model = phenomenological_matrices(codes.bivariate_bicycle_hx(), 12, p, p, logical=tuple(range(12)))
    settings = {f"bpgd_R_{r}_osd0": dict(decimation=dict(round_iters=ROUND_ITERS, max_rounds=r, freeze_llr=FREEZE), decimation_lane_node=True) for r in ROUNDS}
    settings.update(bp30_osd0={}, relay_osd0=dict(relay=RELAY))
    sims = {}
    for leg, kw in settings.items():
        sim = MonteCarloDemSimulation(model, target_run_count=shots, batch_size=batch, seed=5, max_iter=30, bp_method="ms", ms_scaling_factor=0.625, osd_method="osd0", **kw)
        eng = sim._get_engine()
        eng.simulate_b8(5, 0, min(batch, 4096), with_osd=True)  # (untimed: allocations, tables)
        sims[leg] = eng
    rates, counts = {k: [] for k in sims}, {}
    for ps in range(passes):
        for leg, eng in sims.items():
            t0 = time.perf_counter()
            f = u = 0
            for shot0 in range(0, shots, batch):
                df, du = eng.simulate_b8(5, shot0, min(batch, shots - shot0), chunk=min(batch, shots - shot0), with_osd=True)
                f, u = f + df, u + du
            dt = time.perf_counter() - t0
            rates[leg].append(shots / dt)
            counts[leg] = dict(left_for_osd=u, logical_failures=f)
            emit(kind="bpgd_wave_dem", config=f"BB144 x 12 rounds, p = {p}, min-sum, alpha 0.625", leg=leg, run=ps,
                 route=eng.decimation_route(batch) if leg.startswith("bpgd") else None, settings={k: v for k, v in settings[leg].items()}, shots=shots,
                 left_for_osd=u, left_for_osd_counting_error=round(float(np.sqrt(u)), 1), logical_failures=f, logical_error_rate=f / shots,
                 logical_error_rate_se=float(np.sqrt(max(f, 1) * (1 - f / shots)) / shots), shots_per_s=round(shots / dt))
    med, spread = _spread(rates)
    emit(kind="bpgd_wave_dem_summary", config=f"BB144 x 12 rounds, p = {p}", shots=shots, median_shots_per_s={k: round(v) for k, v in med.items()},
         run_to_run_spread={k: round(v, 4) for k, v in spread.items()}, counts=counts)
    for eng in sims.values():
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speed", action="store_true")
    ap.add_argument("--dem", action="store_true")
    ap.add_argument("--bench", default=None, metavar="LIB", help="the parent commit's libldpc_hip.so")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--shots", type=int, default=1 << 20)
    ap.add_argument("--dem-p", type=float, default=0.003)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bench_bpgd._OUT = args.out
    if args.speed:
        speed(args.batch, args.reps, args.warmup, args.passes)
    if args.dem:
        dem(args.shots, args.batch, args.dem_p, args.passes)
    if args.bench:
        bench_bpgd.bench(args.bench, args.passes)


if __name__ == "__main__":
    main()
