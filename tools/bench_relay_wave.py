#!/usr/bin/env python
"""Relay-BP and memory min-sum beyond the lane = edge codes (DESIGN.md sections 7c, 7d): the lane = node route (bp_wave_relay_kernel) against
the per-pass route of the same build, in one process on one box.

    python tools/bench_relay_wave.py --speed     # (a) device-resident, B = 65 536: hgp1600 and hgp400 at p = 0.02
    python tools/bench_relay_wave.py --dem       # (b) BB144 x 12 rounds, p = 0.003, 2^20 shots through simulate_b8
    python tools/bench_relay_wave.py --bench LIB # (c) bench.py --gpus 1 --steps 5 --warmup 2, this build alternating with the build at LIB

The relay is section 7d's: a first leg of 30 iterations at strength 0.125, then 8 legs of 15 with strengths drawn from [-0.24, 0.66], stop at
the first solution; the memory decode: strength 0.35, 30 iterations; min-sum, alpha 0.625.
(a) legs relay_wave / memory_wave (small-code kernel mode 3: the plan's own choice of form) and relay_leg_loop / memory_per_pass (mode 0),
ALTERNATING, every leg ``--passes`` times, each run = ``--warmup`` untimed and ``--reps`` timed decodes of syndromes generated on the device;
one JSON line per leg and pass with the launch log of its decode, and a summary per code: medians, the run-to-run spread of every leg (between
its passes), the ratios, and the rule stated before the measurement -- the lane = node route is the default only if it beats the per-pass route
by more than the spread of the two, on both codes.
(b) the model of tools/bench_relay.py --helps: relay + OSD-0 on the lane = node route, on the leg loop, and min-sum 30 + OSD-0; shots/s, rows
left unsolved (+- sqrt), logical failures (+- the binomial standard error); every leg ``--passes`` times, alternating.
(c) the headline of bench.py, the two builds alternating, ``--passes`` times each.
Lines go to stdout; ``--out FILE`` appends them to a file as well (profiles/relay_wave.jsonl).  Reads nothing but this repository (and LIB).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

_OUT = None
RELAY = dict(gamma0=0.125, pre_iter=30, num_sets=8, set_max_iter=15, gamma_dist_interval=(-0.24, 0.66), stop_nconv=1, seed=0)
MEMORY = 0.35


def emit(**line):
    text = json.dumps(line)
    print(text, flush=True)
    if _OUT:
        with open(_OUT, "a") as f:
            f.write(text + "\n")


def _engine(h, p, relay, mode):
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.relay_decoder import relay_schedule
    h = h.tocsr()
    h.eliminate_zeros()
    h.sort_indices()
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], np.full(h.shape[1], p), 30, 1, 0.625)
    eng.set_small_code_kernel(mode)
    if relay:
        eng.set_relay(*relay_schedule(h.shape[1], **RELAY))
    else:
        eng.set_memory(np.full(h.shape[1], MEMORY))
    return eng


def _summary(kind, config, medians, pairs, **more):
    med = {k: float(np.median(v)) for k, v in medians.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in medians.items()}
    ratios = {}
    for fast, slow in pairs:
        margin = max(spread[fast], spread[slow])
        ratios[f"{fast}_over_{slow}"] = dict(ratio=round(med[fast] / med[slow], 3), margin=round(margin, 4), beats_by_more_than_the_margin=bool(med[fast] / med[slow] - 1 > margin))
    emit(kind=kind, config=config, median_per_s={k: round(v) for k, v in med.items()}, run_to_run_spread={k: round(v, 4) for k, v in spread.items()}, **ratios, **more)


def speed(batch, reps, warmup, passes, p):
    import torch
    from ldpc_amd import codes
    from ldpc_amd.engine import launch_log
    hgp = lambda n: codes.hypergraph_product_hx(codes.regular_ldpc_code(n, 3, 4, seed=5))  # noqa: E731
    for name, h in ((f"hgp1600_p{int(p * 1000):03d}", hgp(32)), (f"hgp400_p{int(p * 1000):03d}", hgp(16))):
        legs = {"relay_wave": _engine(h, p, True, 3), "relay_leg_loop": _engine(h, p, True, 0),
                "memory_wave": _engine(h, p, False, 3), "memory_per_pass": _engine(h, p, False, 0)}
        routes = {k: e.relay_route(batch) for k, e in legs.items()}
        synd = legs["relay_wave"].gen_bsc_syndromes(12345, p, 0, batch, device="cuda")
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
                        kernels = {k: v for k, v in sorted(log.items()) if k.startswith(("bp_", "relay_", "wave_relay"))}
                    else:
                        out = eng.decode_batch(synd, want_llr=False, out=out)
                    torch.cuda.synchronize()
                    if r >= warmup:
                        rates.append(batch / (time.perf_counter() - t0))
                medians[leg].append(float(np.median(rates)))
                emit(kind="relay_wave_speed", config=name, leg=leg, run=ps, route=routes[leg], relay=dict(RELAY) if leg.startswith("relay") else None,
                     memory=None if leg.startswith("relay") else dict(strength=MEMORY, max_iter=30), batch=batch, kernels=kernels,
                     syndromes_per_s=[round(x) for x in rates], median_syndromes_per_s=round(medians[leg][-1]),
                     converged=int(out[3].sum()), mean_iterations=round(float(out[2].double().mean()), 3))
        _summary("relay_wave_speed_summary", name, medians, (("relay_wave", "relay_leg_loop"), ("memory_wave", "memory_per_pass")), batch=batch, routes=routes)
        for eng in legs.values():
            eng.close()


def dem(shots, batch, p, passes):
    from ldpc_amd import codes
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from window_util import phenomenological_matrices
    model = phenomenological_matrices(codes.bivariate_bicycle_hx(), 12, p, p, logical=tuple(range(12)))
    sims = {}
    for leg, relay, mode in (("relay_wave_osd0", RELAY, 3), ("relay_leg_loop_osd0", RELAY, 0), ("bp30_osd0", None, -1)):
        sim = MonteCarloDemSimulation(model, target_run_count=shots, batch_size=batch, seed=5, max_iter=30, bp_method="ms", ms_scaling_factor=0.625,
                                      osd_method="osd0", relay=relay)
        eng = sim._get_engine()
        eng.set_small_code_kernel(mode)
        eng.simulate_b8(5, 0, min(batch, 4096), with_osd=True)  # (untimed: allocations, tables)
        sims[leg] = (eng, relay)
    rates = {k: [] for k in sims}
    for ps in range(passes):
        for leg, (eng, relay) in sims.items():
            t0 = time.perf_counter()
            f = u = 0
            for shot0 in range(0, shots, batch):
                df, du = eng.simulate_b8(5, shot0, min(batch, shots - shot0), chunk=min(batch, shots - shot0), with_osd=True)
                f, u = f + df, u + du
            dt = time.perf_counter() - t0
            rates[leg].append(shots / dt)
            emit(kind="relay_wave_dem", config=f"BB144 x 12 rounds, p = {p}, min-sum, alpha 0.625", leg=leg, run=ps, route=eng.relay_route(batch) if relay else None,
                 relay=relay, shots=shots, unconverged=u, unconverged_counting_error=round(float(np.sqrt(u)), 1), logical_failures=f,
                 logical_error_rate=f / shots, logical_error_rate_se=float(np.sqrt(max(f, 1) * (1 - f / shots)) / shots), shots_per_s=round(shots / dt))
    _summary("relay_wave_dem_summary", f"BB144 x 12 rounds, p = {p}", rates,
             (("relay_wave_osd0", "relay_leg_loop_osd0"), ("relay_wave_osd0", "bp30_osd0")), shots=shots)
    for eng, _ in sims.values():
        eng.close()


def bench(parent_lib, passes):
    values = {"this_build": [], "parent_build": []}
    for ps in range(passes):
        for leg, lib in (("this_build", None), ("parent_build", parent_lib)):
            env = dict(os.environ)
            env.pop("LDPC_HIP_LIB", None)
            if lib:
                env["LDPC_HIP_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"], env=env, capture_output=True, text=True, timeout=600)
            line = json.loads(r.stdout.strip().splitlines()[-1])
            values[leg].append(float(line["value"]))
            emit(kind="relay_wave_bench", leg=leg, run=ps, value=line["value"], metric=line.get("metric"), unit=line.get("unit"))
    _summary("relay_wave_bench_summary", "bench.py --gpus 1 --steps 5 --warmup 2", values, (("this_build", "parent_build"),))


def main():
    global _OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--speed", action="store_true")
    ap.add_argument("--dem", action="store_true")
    ap.add_argument("--bench", default=None, metavar="LIB", help="the parent commit's libldpc_hip.so")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--shots", type=int, default=1 << 20)
    ap.add_argument("--p", type=float, default=0.02)
    ap.add_argument("--dem-p", type=float, default=0.003)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _OUT = args.out
    if args.speed:
        speed(args.batch, args.reps, args.warmup, args.passes, args.p)
    if args.dem:
        dem(args.shots, args.batch, args.dem_p, args.passes)
    if args.bench:
        bench(args.bench, args.passes)


if __name__ == "__main__":
    main()
