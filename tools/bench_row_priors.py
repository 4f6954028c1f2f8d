#!/usr/bin/env python3
"""What per-row channel probabilities (decode_batch(..., channel_probs=P)) cost against the SAME build's shared-prior decode on the SAME
forced kernel, timed in one process, the two interleaved call by call:

  * the headline code ((3,6)-regular, n = 10 000, product-sum 50 at p = 0.05), B = 4 096, per-pass kernels forced (set_handoff above
    the tile count: the path a row-prior decode takes), plain against row priors;
  * BB [[144,12,12]] hx, product-sum 50 at p = 0.05, B = 8 192, slot kernel forced (set_small_code_kernel 2), plain against row priors.

Every row of P is the handle's own probability, so both sides do the same arithmetic and must return the same bits (checked); the
difference is the priors' traffic: a conversion pass and one 512-byte segment per bit per bit pass (per-pass kernels), a strided read
per slot refill (slot kernel).  Also printed: the box's copy-probe rate from the same run.  No threshold: numbers for NOTES.md.
Run on an MI355X:   python tools/bench_row_priors.py [--reps 7]

--edge: the lane = edge codes, min-sum, where a row-prior decode may run on bp_edge_rp_kernel / bp_edge8_rp_kernel (debug switch EDGE_RP) or on
the slot kernel: BB [[144,12,12]] hx min-sum 50 at p = 0.05, B = 65 536, and the rotated surface code d = 21, min-sum 30 at p = 0.05,
B = 262 144, device-resident, three untimed decodes and then the median of --reps (>= 7) timed ones.  One process is one LEG; a job runs

    python tools/bench_row_priors.py --edge --leg row_priors --tree <parent checkout> --tree-name parent   >> lines.jsonl    # 1
    python tools/bench_row_priors.py --edge --leg row_priors --edge-rp 1                                    >> lines.jsonl    # 2
    python tools/bench_row_priors.py --edge --leg row_priors --edge-rp 0                                    >> lines.jsonl    # 3
    python tools/bench_row_priors.py --edge --leg plain                                                     >> lines.jsonl    # 4
    python tools/bench_row_priors.py --edge --leg row_priors --tree <parent checkout> --tree-name parent   >> lines.jsonl    # 5
    python tools/bench_row_priors.py --edge-verdict lines.jsonl

Every row of P is the handle's own probability, so all legs do the same arithmetic: each line carries a checksum of its outputs, and the
verdict refuses lines of one configuration whose checksums differ.  Each line also names the BP kernels its decode launched (where the
tree has a launch log).  The verdict applies the rule of DESIGN.md section 4: the route becomes the default if leg 2 beats the better of the
parent's two figures on BOTH codes by more than the spread between those two figures.

--wave: the lane = node codes, min-sum 30, alpha 0.625, B = 65 536, device-resident, where a row-prior decode may run on bp_wave_rp_kernel (debug
switch WAVE_RP), on the slot kernel or on the per-pass kernels: HGP [[400,16]] and the [[1600,64]] hypergraph product at p = 0.02, and the BB144 x
12 rounds detector error model (864 x 2520) at p = 0.003 with its own priors.  One process is one leg; a job alternates them, every leg twice:

    python tools/bench_row_priors.py --wave --leg row_priors --tree <parent checkout> --tree-name parent   >> lines.jsonl
    python tools/bench_row_priors.py --wave --leg row_priors --wave-rp 1                                    >> lines.jsonl
    python tools/bench_row_priors.py --wave --leg row_priors --wave-rp 0                                    >> lines.jsonl
    python tools/bench_row_priors.py --wave --leg plain                                                     >> lines.jsonl    # the ceiling: bp_wave_kernel
    ... the four once more ...
    python tools/bench_row_priors.py --wave-verdict lines.jsonl

The verdict applies the rule of DESIGN.md section 4: the route becomes the default of modes -1, 1 and 6 if the slower of its two runs beats the
better of the parent's two on ALL THREE codes by more than the larger of the two legs' run-to-run spreads."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

# --tree DIR: take ldpc_amd (and its built library) from another checkout -- it must be on the path before the first import of the package
_pre = argparse.ArgumentParser(add_help=False)
_pre.add_argument("--tree", default=None)
sys.path.insert(0, os.path.abspath(_pre.parse_known_args()[0].tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
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


BP_KERNELS = ("bp_wave_rp_kernel", "wave_rp_prior_kernel", "bp_spread_init_kernel", "bp_edge_rp_kernel", "bp_edge8_rp_kernel", "bp_edge_kernel", "bp_edge8_kernel", "bp_small_kernel", "bp_wave_kernel", "bp_wave_ps_kernel",
              "bp_decode_kernel", "bp_spread_check_kernel", "bp_spread_bit_kernel", "row_priors_kernel", "row_priors_rowmajor_kernel")


def edge_leg(args):
    """One leg of the --edge measurement: both codes, one JSON line each."""
    try:
        from ldpc_amd.engine import launch_log
    except ImportError:  # (a tree from before the launch log)
        launch_log = None
    for name, h, max_iter, batch in (("bb144_ms50_p050", codes.bivariate_bicycle_hx(), 50, 65536),
                                     ("surface21_ms30_p050", codes.rotated_surface_code_x(21), 30, 262144)):
        h = sp.csr_matrix(h)
        h.sort_indices()
        m, n = h.shape
        p = 0.05
        eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, p), max_iter, 1, 0.625)
        if args.edge_rp >= 0:
            eng.set_debug_switch("EDGE_RP", args.edge_rp)
        s = eng.gen_bsc_syndromes(7, p, shot0=0, shots=batch, device="cuda:0")
        kw = {"channel_probs": torch.full((batch, n), p, dtype=torch.float64, device="cuda:0")} if args.leg == "row_priors" else {}
        kernels = None
        if launch_log is not None:
            with launch_log() as log:
                eng.decode_batch(s, **kw)
                torch.cuda.synchronize()
            kernels = sorted(k for k in log if k.split("<")[0] in BP_KERNELS)
        for _ in range(3):  # untimed
            out = eng.decode_batch(s, asynchronous=True, **kw)
            torch.cuda.synchronize()
        digest = hashlib.sha256()
        for o in out:
            digest.update(o.cpu().numpy().tobytes())
        wall, kern = [], []
        for _ in range(max(args.reps, 7)):
            t0 = time.perf_counter()
            eng.decode_batch(s, asynchronous=True, **kw)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(eng.last_kernel_ms())
        med = float(np.median(wall))
        print(json.dumps({"config": name, "leg": args.leg, "tree": args.tree_name or (args.tree or "this"), "edge_rp": args.edge_rp, "m": m, "n": n,
                          "batch": batch, "max_iter": max_iter, "p": p, "reps": len(wall), "mean_iterations": round(float(out[2].float().mean()), 3),
                          "converged": round(float(out[3].float().mean()), 4), "wall_ms_median": round(med, 4),
                          "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4), "bp_kernel_ms_median": round(float(np.median(kern)), 4),
                          "syndromes_per_s": round(batch / med * 1e3), "outputs_sha256_16": digest.hexdigest()[:16], "bp_kernels": kernels}), flush=True)
        eng.close()
        del s, kw, out
        torch.cuda.empty_cache()


def edge_verdict(path):
    """The rule on the lines of one job (legs in the order of the module docstring)."""
    lines = [json.loads(x) for x in open(path) if x.startswith("{")]
    ok, wins = True, []
    for cfg in sorted({x["config"] for x in lines}):
        rows = [x for x in lines if x["config"] == cfg]
        if len({x["outputs_sha256_16"] for x in rows}) != 1:
            print(f"{cfg}: MISMATCH -- the legs' outputs differ: {[(x['tree'], x['leg'], x['edge_rp'], x['outputs_sha256_16']) for x in rows]}")
            ok = False
            continue
        parent = [x["syndromes_per_s"] for x in rows if x["tree"] == "parent" and x["leg"] == "row_priors"]
        on = [x["syndromes_per_s"] for x in rows if x["tree"] != "parent" and x["leg"] == "row_priors" and x["edge_rp"] == 1]
        off = [x["syndromes_per_s"] for x in rows if x["tree"] != "parent" and x["leg"] == "row_priors" and x["edge_rp"] == 0]
        plain = [x["syndromes_per_s"] for x in rows if x["tree"] != "parent" and x["leg"] == "plain"]
        if len(parent) != 2 or len(on) != 1:
            print(f"{cfg}: incomplete job: parent {parent}, EDGE_RP = 1 {on}")
            ok = False
            continue
        spread = abs(parent[0] - parent[1])
        win = on[0] > max(parent) + spread
        wins.append(win)
        print(json.dumps({"config": cfg, "identical_outputs": True, "parent_row_priors": parent, "parent_spread": spread, "edge_rp_1": on[0],
                          "edge_rp_0": off[0] if off else None, "plain": plain[0] if plain else None,
                          "edge_rp_1_over_best_parent": round(on[0] / max(parent), 4),
                          "edge_rp_1_over_plain": round(on[0] / plain[0], 4) if plain else None, "beats_parent_by_more_than_spread": bool(win)}))
    print("RULE: " + ("the lane = edge route becomes the default" if ok and len(wins) == 2 and all(wins) else "the default stays the slot kernel"))
    return ok


def _wave_configs():
    """(name, h, the handle's probabilities, p): the codes of --wave."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from window_util import phenomenological_matrices
    hgp = lambda n: codes.hypergraph_product_hx(codes.regular_ldpc_code(n, 3, 4, seed=5))  # noqa: E731
    check, _, pri = phenomenological_matrices(codes.bivariate_bicycle_hx(), 12, 0.003, 0.003, logical=tuple(range(12)))
    return [("hgp400_ms30_p020", hgp(16), None, 0.02), ("hgp1600_ms30_p020", hgp(32), None, 0.02),
            ("bb144x12_dem_ms30_p003", check, np.clip(np.asarray(pri, np.float64), 1e-9, 1 - 1e-9), 0.003)]


def wave_leg(args):
    """One leg of the --wave measurement: the three codes, one JSON line each.  Every row of P is the handle's own probabilities."""
    try:
        from ldpc_amd.engine import launch_log
    except ImportError:
        launch_log = None
    batch, max_iter = 65536, 30
    for name, h, pri, p in _wave_configs():
        h = sp.csr_matrix(h)
        h.eliminate_zeros()
        h.sort_indices()
        m, n = h.shape
        own = np.full(n, p) if pri is None else pri
        eng = HipBpEngine(h.indptr, h.indices, n, own, max_iter, 1, 0.625)
        if args.wave_rp >= 0:
            eng.set_debug_switch("WAVE_RP", args.wave_rp)
        if pri is None:
            s = eng.gen_bsc_syndromes(12345, p, shot0=0, shots=batch, device="cuda:0")
        else:
            eng.set_sampler(pri)
            s = eng.unpack_b8(eng.sample_b8(12345, 0, batch, device="cuda")[0], m).contiguous()
        kw = {"channel_probs": torch.from_numpy(own).cuda().repeat(batch, 1).contiguous()} if args.leg == "row_priors" else {}
        route = eng.row_prior_route(batch) if args.leg == "row_priors" and hasattr(eng, "row_prior_route") else None
        kernels = None
        if launch_log is not None:
            with launch_log() as log:
                eng.decode_batch(s, **kw)
                torch.cuda.synchronize()
            kernels = {k: v for k, v in sorted(log.items()) if k.split("<")[0] in BP_KERNELS}
        for _ in range(2):  # untimed
            out = eng.decode_batch(s, asynchronous=True, **kw)
            torch.cuda.synchronize()
        digest = hashlib.sha256()
        for o in out:
            digest.update(o.cpu().numpy().tobytes())
        wall, kern = [], []
        for _ in range(max(args.reps, 5)):
            t0 = time.perf_counter()
            eng.decode_batch(s, asynchronous=True, **kw)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(eng.last_kernel_ms())
        med = float(np.median(wall))
        print(json.dumps({"kind": "row_priors_wave", "config": name, "leg": args.leg, "tree": args.tree_name or (args.tree or "this"), "wave_rp": args.wave_rp,
                          "route": route, "m": m, "n": n, "batch": batch, "max_iter": max_iter, "p": p, "reps": len(wall),
                          "mean_iterations": round(float(out[2].float().mean()), 3), "converged": round(float(out[3].float().mean()), 4),
                          "wall_ms_median": round(med, 4), "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4),
                          "bp_kernel_ms_median": round(float(np.median(kern)), 4), "syndromes_per_s": round(batch / med * 1e3),
                          "outputs_sha256_16": digest.hexdigest()[:16], "bp_kernels": kernels}), flush=True)
        eng.close()
        del s, kw, out
        torch.cuda.empty_cache()


def wave_verdict(path):
    """The rule on the lines of one job."""
    lines = [x for x in (json.loads(x) for x in open(path) if x.startswith("{")) if x.get("kind") == "row_priors_wave"]
    ok, wins = True, []
    for cfg in sorted({x["config"] for x in lines}):
        rows = [x for x in lines if x["config"] == cfg]
        if len({x["outputs_sha256_16"] for x in rows}) != 1:
            print(f"{cfg}: MISMATCH -- the legs' outputs differ: {[(x['tree'], x['leg'], x['wave_rp'], x['outputs_sha256_16']) for x in rows]}")
            ok = False
            continue
        rate = lambda f: [x["syndromes_per_s"] for x in rows if f(x)]  # noqa: E731
        parent = rate(lambda x: x["tree"] == "parent" and x["leg"] == "row_priors")
        on = rate(lambda x: x["tree"] != "parent" and x["leg"] == "row_priors" and x["wave_rp"] == 1)
        off = rate(lambda x: x["tree"] != "parent" and x["leg"] == "row_priors" and x["wave_rp"] == 0)
        plain = rate(lambda x: x["tree"] != "parent" and x["leg"] == "plain")
        if len(parent) < 2 or len(on) < 2:
            print(f"{cfg}: incomplete job: parent {parent}, WAVE_RP = 1 {on}")
            ok = False
            continue
        margin = max(max(parent) - min(parent), max(on) - min(on))
        win = min(on) > max(parent) + margin
        wins.append(win)
        print(json.dumps({"config": cfg, "identical_outputs": True, "parent_row_priors": parent, "wave_rp_1": on, "wave_rp_0": off, "plain_bp_wave_kernel": plain,
                          "margin": margin, "wave_rp_1_over_best_parent": round(min(on) / max(parent), 3),
                          "wave_rp_1_over_plain": round(float(np.median(on)) / float(np.median(plain)), 3) if plain else None,
                          "beats_parent_by_more_than_the_spread": bool(win)}))
    print("RULE: " + ("the lane = node route becomes the default" if ok and len(wins) == 3 and all(wins) else "the default stays (slot kernel / per-pass kernels)"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--edge", action="store_true", help="one leg of the lane = edge measurement (see the module docstring)")
    ap.add_argument("--leg", default="row_priors", choices=["row_priors", "plain"])
    ap.add_argument("--edge-rp", type=int, default=-1, help="--edge: debug switch EDGE_RP (-1: leave it unset -- the tree's default; a tree without the switch)")
    ap.add_argument("--wave", action="store_true", help="one leg of the lane = node measurement (see the module docstring)")
    ap.add_argument("--wave-rp", type=int, default=-1, help="--wave: debug switch WAVE_RP (-1: leave it unset -- the tree's default; a tree without the switch)")
    ap.add_argument("--wave-verdict", metavar="JSONL", default=None, help="apply the lane = node rule to the lines of one job")
    ap.add_argument("--tree", default=None, help="another built checkout to take ldpc_amd from (default: this one)")
    ap.add_argument("--tree-name", default=None, help="what the lines call the tree")
    ap.add_argument("--edge-verdict", metavar="JSONL", default=None, help="apply the rule to the lines of one job")
    args = ap.parse_args()
    if args.edge_verdict:
        sys.exit(0 if edge_verdict(args.edge_verdict) else 1)
    if args.wave_verdict:
        sys.exit(0 if wave_verdict(args.wave_verdict) else 1)
    if args.edge:
        edge_leg(args)
        return
    if args.wave:
        wave_leg(args)
        return
    ok = pair("headline (3,6) n=10000 ps50, per-pass forced", codes.regular_ldpc_code(10000, 3, 6, seed=1), 0.05, 50, 4096,
              lambda e: (e.set_handoff(1 << 20), e.set_repack(0)), args.reps)
    ok &= pair("BB144 hx ps50, slot kernel forced", codes.bivariate_bicycle_hx(), 0.05, 50, 8192, lambda e: e.set_small_code_kernel(2), args.reps)
    print("IDENTICAL" if ok else "MISMATCH")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
