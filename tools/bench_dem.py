#!/usr/bin/env python3
"""What sampling a detector error model on the device buys: the sample -> decode -> compare loop of HipBpEngine.simulate_b8 against its parts
and against the same job with the shots sampled on the host.

Model: the tools/bench_window.py model (BB [[144,12,12]] hx x 12 rounds, phenomenological noise, 864 detectors x 2520 errors), decoded whole
with min-sum 30 iterations + OSD-0.  2^20 shots in chunks of 65 536; three untimed chunks, then every leg twice, alternating:

  a  sample_b8 alone (device tensors out)
  b  decode_b8 alone, on detection events that are on the device already
  c  simulate_b8: sample, decode, predict observables, count -- two counters come back
  d  the same job without the device sampler: noise_models.generate_dem_batch on the host, decode_b8 from NumPy arrays, compare on the host;
     the host sampling is timed on its own as well as included

  e  (beside the issue's four) leg d's device share on its own: decode_b8 from NumPy arrays that were sampled beforehand + the host compare,
     back to back -- what leg d's decode_and_compare_seconds would be if the device were not left idle while the host samples

One JSON line per leg goes to --out (default profiles/dem_simulate.jsonl), then one with the launch log of a single simulate_b8 chunk, then
a summary: c / b, c / d, a's share of c, and the run-to-run spread of b (the distance of its two legs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1 << 20)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--p", type=float, default=0.003)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--host-block", type=int, default=8192, help="shots per generate_dem_batch call of leg d (bounds the host's memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dem_simulate.jsonl"))
    args = ap.parse_args()
    import scipy.sparse as sp
    import torch
    from ldpc_amd import codes
    from ldpc_amd.engine import HipBpEngine, launch_log
    from ldpc_amd.noise_models import generate_dem_batch
    from window_util import phenomenological_matrices

    h = codes.bivariate_bicycle_hx()
    rounds = 12
    check, obs, pri = phenomenological_matrices(h, rounds, args.p, args.p, logical=tuple(range(12)))
    check = sp.csr_matrix(check, dtype=np.uint8)
    check.sort_indices()
    m, n = check.shape
    k = obs.shape[0]
    eng = HipBpEngine(check.indptr, check.indices, n, pri, 30, 1, 0.625)
    eng.set_osd(1, 0)
    eng.set_observables(obs)
    eng.set_sampler(pri)
    dev = torch.device("cuda", torch.cuda.current_device())
    shots, chunk, seed = args.shots, args.chunk, args.seed
    starts = list(range(0, shots, chunk))
    config = f"BB144 x {rounds} rounds ({m} x {n}), min_sum 30 it + OSD-0, p={args.p}, {shots} shots in chunks of {chunk}"

    def host_sample(s0, count):
        parts = [generate_dem_batch(check, obs, pri, seed, s0 + q, min(args.host_block, count - q))[1:] for q in range(0, count, args.host_block)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    # device-resident detection events of the whole run for leg b; three untimed chunks of everything
    dets_all = torch.cat([eng.sample_b8(seed, s0, min(chunk, shots - s0), device=dev)[0] for s0 in starts])
    warm_d, warm_o = host_sample(0, min(chunk, shots))
    for _ in range(3):
        eng.sample_b8(seed, 0, chunk, device=dev)
        eng.decode_b8(dets_all[:chunk], with_osd=True)
        eng.simulate_b8(seed, 0, chunk, chunk=chunk, with_osd=True)
        eng.decode_b8(warm_d, with_osd=True)
    torch.cuda.synchronize()

    def leg_a():
        t0 = time.perf_counter()
        for s0 in starts:
            eng.sample_b8(seed, s0, min(chunk, shots - s0), device=dev)
        torch.cuda.synchronize()
        return {"seconds": time.perf_counter() - t0}

    def leg_b():
        t0 = time.perf_counter()
        for s0 in starts:
            eng.decode_b8(dets_all[s0:s0 + chunk], with_osd=True)
        torch.cuda.synchronize()
        return {"seconds": time.perf_counter() - t0}

    def leg_c():
        t0 = time.perf_counter()
        fails, unconverged = eng.simulate_b8(seed, 0, shots, chunk=chunk, with_osd=True)
        return {"seconds": time.perf_counter() - t0, "fail_count": fails, "bp_unconverged_count": unconverged}

    def leg_d():
        t_sample = t_rest = 0.0
        fails = unconverged = 0
        for s0 in starts:
            t0 = time.perf_counter()
            dets, true_obs = host_sample(s0, min(chunk, shots - s0))
            t1 = time.perf_counter()
            pred, _, _, conv = eng.decode_b8(dets, with_osd=True)
            fails += int(np.count_nonzero((pred != true_obs).any(axis=1)))
            unconverged += int(np.count_nonzero(~conv))
            t_sample += t1 - t0
            t_rest += time.perf_counter() - t1
        return {"seconds": t_sample + t_rest, "host_sampling_seconds": t_sample, "decode_and_compare_seconds": t_rest, "fail_count": fails,
                "bp_unconverged_count": unconverged}

    presampled = []  # (filled before the timed legs) the first chunks of the run as host arrays, for leg e

    def leg_e():
        t0 = time.perf_counter()
        fails = 0
        for dets, true_obs in presampled:
            pred, _, _, conv = eng.decode_b8(dets, with_osd=True)
            fails += int(np.count_nonzero((pred != true_obs).any(axis=1)))
        dt = time.perf_counter() - t0
        return {"seconds": dt * len(starts) / len(presampled), "measured_chunks": len(presampled), "seconds_per_chunk": dt / len(presampled)}

    for s0 in starts[:4]:
        d, o = eng.sample_b8(seed, s0, min(chunk, shots - s0))  # (NumPy out: the sample of leg d, bit for bit)
        presampled.append((d, o))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d, "e": leg_e}
    what = {"a": "sample_b8 alone", "b": "decode_b8 on device-resident detection events", "c": "simulate_b8",
            "d": "generate_dem_batch on the host + decode_b8 from NumPy + compare on the host",
            "e": "decode_b8 from pre-sampled NumPy arrays + compare on the host, back to back (4 chunks, scaled to the run)"}
    results = {name: [] for name in legs}
    with open(args.out, "w") as f:
        for rep in range(2):
            for name, fn in legs.items():
                r = fn()
                r.update(leg=name, what=what[name], rep=rep, config=config, shots=shots, shots_per_s=shots / r["seconds"])
                results[name].append(r)
                f.write(json.dumps(r) + "\n")
                f.flush()
                print(json.dumps(r))
        with launch_log() as log:
            eng.simulate_b8(seed, 0, min(chunk, shots), chunk=chunk, with_osd=True)
        f.write(json.dumps({"launch_log_of_one_simulate_b8_chunk": log, "chunk": min(chunk, shots)}) + "\n")
        best = {name: min(r["seconds"] for r in rs) for name, rs in results.items()}
        spread_b = abs(results["b"][0]["seconds"] - results["b"][1]["seconds"])
        summary = {"summary": config, "seconds_best_of_two": best, "c_over_b": best["c"] / best["b"], "c_over_d": best["c"] / best["d"],
                   "d_minus_c_seconds": best["d"] - best["c"], "a_share_of_c": best["a"] / best["c"], "spread_of_b_seconds": spread_b,
                   "c_beats_d_by_more_than_the_spread": bool(best["d"] - best["c"] > spread_b),
                   "d_host_sampling_seconds": min(r["host_sampling_seconds"] for r in results["d"]),
                   "d_decode_and_compare_seconds": min(r["decode_and_compare_seconds"] for r in results["d"]),
                   "e_seconds_scaled_to_the_run": best["e"],
                   "counts_agree": len({(r["fail_count"], r["bp_unconverged_count"]) for r in results["c"] + results["d"]}) == 1}
        f.write(json.dumps(summary) + "\n")
        print(json.dumps(summary))


if __name__ == "__main__":
    main()
