#!/usr/bin/env python
"""BP with guided decimation (ldpc_hip_bp_set_decimation): what it costs and how many rows it solves.

    python tools/bench_bpgd.py --out profiles/bpgd.jsonl              # the decode legs
    python tools/bench_bpgd.py --bench LIB --out profiles/bpgd.jsonl  # bench.py --gpus 1 --steps 5 --warmup 2, this build alternating with the build at LIB (the parent commit's library)

BB144 ``hx`` and the rotated surface code d = 21, min-sum alpha 0.625, B = 65 536, p = 0.05, syndromes generated on the device, everything in
HBM.  The legs: plain min-sum 30; plain min-sum at BPGD's worst-case budget (5 n iterations); the relay of DESIGN.md section 7d(a) (30
iterations at strength 0.125, then 8 legs of 15 drawn from [-0.24, 0.66], stop at the first solution); BPGD T = 5, C = 25 with R = n and
with R = 16.  One process, one engine per leg, the legs ALTERNATING and every one run ``--passes`` times (default 2), each run = ``--warmup`` untimed
decodes and ``--reps`` timed ones; one JSON line per leg and pass with the kernels its decode launched (the launch log, taken in an untimed decode of its own), rows solved and mean
iterations per row, and a summary line per code: the medians and the run-to-run spread of every leg (between its passes).  Nothing is
gated on these figures.  Lines go to stdout; ``--out FILE`` appends them to a file as well.  Reads nothing but this repository (and LIB).
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

_OUT = None
RELAY = dict(gamma0=0.125, pre_iter=30, num_sets=8, set_max_iter=15, gamma_dist_interval=(-0.24, 0.66), stop_nconv=1, seed=0)
ROUND_ITERS, FREEZE = 5, 25.0


def emit(**line):
    text = json.dumps(line)
    print(text, flush=True)
    if _OUT:
        with open(_OUT, "a") as f:
            f.write(text + "\n")


def _engine(h, p, max_iter, relay=None, decimation=None):
    from ldpc_amd.engine import HipBpEngine
    from ldpc_amd.relay_decoder import relay_schedule
    h = h.tocsr()
    h.sort_indices()
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], np.full(h.shape[1], p), max_iter, 1, 0.625)
    if relay is not None:
        eng.set_relay(*relay_schedule(h.shape[1], **relay))
    if decimation is not None:
        eng.set_decimation(*decimation)
    return eng


def speed(batch, reps, warmup, passes, p):
    import torch
    from ldpc_amd import codes
    from ldpc_amd.engine import launch_log
    for name, h in (("bb144_p050", codes.bivariate_bicycle_hx()), ("surface_d21_p050", codes.rotated_surface_code_x(21))):
        n = h.shape[1]
        settings = {"plain_30": dict(max_iter=30), "plain_worst_case_budget": dict(max_iter=ROUND_ITERS * n), "relay": dict(max_iter=30, relay=RELAY),
                    "bpgd_R_n": dict(max_iter=30, decimation=(ROUND_ITERS, n, FREEZE)), "bpgd_R_16": dict(max_iter=30, decimation=(ROUND_ITERS, 16, FREEZE))}
        legs = {k: _engine(h, p, **kw) for k, kw in settings.items()}
        synd = legs["plain_30"].gen_bsc_syndromes(12345, p, 0, batch, device="cuda")
        medians = {k: [] for k in legs}
        solved = {}
        for ps in range(passes):
            for leg, eng in legs.items():  # alternating: every pass visits every leg
                rates = []
                with launch_log() as log:  # (an untimed decode of its own carries the log hook)
                    out = eng.decode_batch(synd, want_llr=False)
                    torch.cuda.synchronize()
                kernels = {k: v for k, v in sorted(log.items()) if k.startswith(("bp_", "relay_", "edge_"))}
                for r in range(reps + warmup):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = eng.decode_batch(synd, want_llr=False, out=out)
                    torch.cuda.synchronize()
                    if r >= warmup:
                        rates.append(batch / (time.perf_counter() - t0))
                medians[leg].append(float(np.median(rates)))
                solved[leg] = int(out[3].sum())
                kw = settings[leg]
                emit(kind="bpgd_speed", config=name, leg=leg, run=ps, max_iter=None if len(kw) > 1 else kw["max_iter"], relay=kw.get("relay"),
                     decimation=kw.get("decimation"), batch=batch, p=p, kernels=kernels, syndromes_per_s=[round(x) for x in rates],
                     median_syndromes_per_s=round(medians[leg][-1]), converged=solved[leg], mean_iterations=round(float(out[2].double().mean()), 3))
        med = {k: float(np.median(v)) for k, v in medians.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in medians.items()}
        emit(kind="bpgd_speed_summary", config=name, batch=batch, p=p, median_syndromes_per_s={k: round(v) for k, v in med.items()},
             run_to_run_spread={k: round(v, 4) for k, v in spread.items()}, rows_solved=solved,
             bpgd_solves_more_rows_than_the_relay=bool(solved["bpgd_R_n"] > solved["relay"]))
        for eng in legs.values():
            eng.close()


def bench(parent_lib, passes):
    """bench.py's headline, this build alternating with the build at ``parent_lib``, ``passes`` times each."""
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
            emit(kind="bpgd_bench", leg=leg, run=ps, value=line["value"], metric=line.get("metric"), unit=line.get("unit"))
    med = {k: float(np.median(v)) for k, v in values.items()}
    emit(kind="bpgd_bench_summary", command="bench.py --gpus 1 --steps 5 --warmup 2", median={k: round(v) for k, v in med.items()},
         run_to_run_spread={k: round((max(v) - min(v)) / med[k], 4) for k, v in values.items()}, this_over_parent=round(med["this_build"] / med["parent_build"], 4))


def main():
    global _OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--speed", action="store_true", help="the decode legs (the default when --bench is not given)")
    ap.add_argument("--bench", default=None, metavar="LIB", help="the parent commit's libldpc_hip.so: bench.py on this build and on that one, alternating")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _OUT = args.out
    if args.speed or not args.bench:
        speed(args.batch, args.reps, args.warmup, args.passes, args.p)
    if args.bench:
        bench(args.bench, args.passes)


if __name__ == "__main__":
    main()
