#!/usr/bin/env python
"""float32 message mode against float64: agreement of the results, and speed.

    python tools/bench_f32.py --agreement                 # share of rows whose decisions / converge flags differ between the modes
    python tools/bench_f32.py --speed                     # syndromes/s of both modes + the copy probe, same process, same box
    python tools/bench_f32.py --speed --modes float64 --tree <checkout>   # the float64 of another built checkout (the parent commit: A/B on one box)
    python tools/bench_f32.py --speed --configs small     # the small codes the on-chip kernels take (each at its own batch sizes)
    python tools/bench_f32.py --speed --repack 0          # ... with the two-pass decode off (set_repack; default -1: the previous decode's histogram decides)
    python tools/bench_f32.py --agreement-two-pass        # float32 two-pass against float32 with set_repack(0): rows that differ, log-ratio bits included
    python tools/bench_f32.py --speed --configs node --modes float32_lane_node,float64   # the codes beyond the lane = edge kernels, float32 on the lane = node kernel

Configurations: (3,6)-regular n = 10 000, min-sum 50 iterations, at p = 0.05 and 0.09; the irregular n = 10 000 code of
``bench.py --full`` (speed only); BB144 min-sum 50 + OSD-0 (agreement only).  ``--configs small`` (speed only): the codes whose messages
stay on chip in both modes -- BB144 min-sum 50 at p = 0.05 (B = 65 536 and 262 144; bp_edge8, DC 3), the rotated surface code d = 21 min-sum
30 at p = 0.05 (B = 262 144; bp_edge) and the hypergraph product of hamming_code(3) with itself min-sum 30 at p = 0.05 (B = 262 144;
bp_edge8, DC 4); every line names the BP kernels its decode launched (``bp_kernels``, from the launch log), so the route is on record.
``--configs node`` (speed, and the rows that differ between the modes of one call): the codes beyond the lane = edge ladders, which FP64
decodes with bp_wave_kernel -- the hypergraph products [[400,16]] and [[1600,64]] of tools/bench_relay_wave.py at p = 0.02 min-sum 30, BB288
at p = 0.05 min-sum 30, and the BB144 x 12 rounds detector error model of tools/bench_dem.py (864 x 2520) at p = 0.003 min-sum 30 + OSD-0, at
``--batch`` rows; modes ``float32`` (the switch off: per-pass), ``float32_lane_node`` (ldpc_hip_bp_set_f32_lane_node on) and ``float64``.
Syndromes are generated on the device; everything stays in HBM.  One JSON line per figure.  Reads nothing but this
repository.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

# --tree DIR: take ldpc_amd (and its built library) from another checkout -- it must be on the path before the first import of the package
_pre = argparse.ArgumentParser(add_help=False)
_pre.add_argument("--tree", default=None)
_TREE = os.path.abspath(_pre.parse_known_args()[0].tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _TREE)


def _engine(h, p, max_iter, alpha=0.625):
    from ldpc_amd.engine import HipBpEngine
    h = h.tocsr()
    h.sort_indices()
    return HipBpEngine(h.indptr, h.indices, h.shape[1], np.full(h.shape[1], p), max_iter, 1, alpha)


def _configs(which):
    from ldpc_amd import codes
    out = []
    if "ldpc36" in which:
        h = codes.regular_ldpc_code(10000, 3, 6, seed=1)
        out += [("ldpc36_n10000_ms50_p050", h, 0.05, False), ("ldpc36_n10000_ms50_p090", h, 0.09, False)]
    if "irregular" in which:
        out += [("irregular_n10000_ms50_p030", codes.irregular_ldpc_code(10000, 5000, seed=1), 0.03, False)]
    if "bb144" in which:
        out += [("bb144_ms50_osd0_p050", codes.bivariate_bicycle_hx(), 0.05, True)]
    return out


def _small_configs():
    """(name, h, p, max_iter, batches): small codes of the lane = edge families, device-resident."""
    from ldpc_amd import codes
    hgp = codes.hypergraph_product_hx(codes.hamming_code(3)).tocsr()
    hgp.eliminate_zeros()  # (the product stores explicit zeros and the engine takes the STRUCTURE; without them: 21 rows of 5 .. 7 entries, columns of 1 .. 4)
    return [("bb144_ms50_p050", codes.bivariate_bicycle_hx(), 0.05, 50, (65536, 262144)),
            ("surface_d21_ms30_p050", codes.rotated_surface_code_x(21), 0.05, 30, (262144,)),
            ("hgp_hamming3_ms30_p050", hgp, 0.05, 30, (262144,))]


def speed_small(modes, reps, warmup, tag, tree_name=None):
    """Small codes: one on-chip launch per decode in float64, and in float32 where the tree has the on-chip float32 kernels (else the
    per-pass route).  `warmup` untimed decodes, then `reps` timed ones; wall time around a synchronised call and the kernel's own time."""
    import torch
    try:
        from ldpc_amd.engine import launch_log as _launch_log
    except ImportError:  # (a checkout from before the launch log)
        _launch_log = None
    assert warmup >= 1
    for name, h, p, max_iter, batches in _small_configs():
        eng = _engine(h, p, max_iter)
        for batch in batches:
            synd = eng.gen_bsc_syndromes(12345, p, 0, batch, device="cuda")
            for mode in modes:
                if mode != "float64" or hasattr(eng, "set_message_dtype"):
                    eng.set_message_dtype(mode)
                out = None
                rates, kms = [], []
                kernels = None
                for r in range(reps + warmup):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if r == 0 and _launch_log is not None:  # (an untimed decode: which BP kernels it launched, and how often)
                        with _launch_log() as log:
                            out = eng.decode_batch(synd, want_llr=False, out=out)
                            torch.cuda.synchronize()
                        kernels = {k: v for k, v in sorted(log.items()) if k.startswith("bp_")}
                    else:
                        out = eng.decode_batch(synd, want_llr=False, out=out)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if r >= warmup:
                        rates.append(batch / dt)
                        kms.append(eng.last_kernel_ms())
                print(json.dumps(dict(kind="speed_small", config=name, mode=mode, tree=tree_name or os.path.relpath(_TREE), tag=tag, batch=batch, bp_kernels=kernels,
                                      syndromes_per_s=[round(x) for x in rates], median_syndromes_per_s=round(float(np.median(rates))),
                                      min_syndromes_per_s=round(min(rates)), max_syndromes_per_s=round(max(rates)),
                                      kernel_ms=[round(x, 3) for x in kms], converged=int(out[3].sum()),
                                      mean_iterations=round(float(out[2].double().mean()), 3))), flush=True)
        eng.close()


def _node_configs():
    """(name, h, priors, p, osd): the codes of --configs node; the detector error model comes with its own priors and is decoded with OSD-0."""
    from ldpc_amd import codes
    sys.path.insert(0, os.path.join(_TREE, "tests"))
    from window_util import phenomenological_matrices
    hgp = lambda n: codes.hypergraph_product_hx(codes.regular_ldpc_code(n, 3, 4, seed=5))  # noqa: E731
    bb288 = codes.bivariate_bicycle_hx(12, 12, (("x", 3), ("y", 2), ("y", 7)), (("y", 3), ("x", 1), ("x", 2)))
    check, _, pri = phenomenological_matrices(codes.bivariate_bicycle_hx(), 12, 0.003, 0.003, logical=tuple(range(12)))
    return [("hgp400_ms30_p020", hgp(16), None, 0.02, False), ("hgp1600_ms30_p020", hgp(32), None, 0.02, False), ("bb288_ms30_p050", bb288, None, 0.05, False),
            ("bb144x12_dem_ms30_osd0_p003", check, np.asarray(pri, np.float64), 0.003, True)]


def speed_node(batch, modes, reps, warmup, tag, tree_name=None):
    """The codes beyond the lane = edge ladders: `warmup` untimed decodes, then `reps` timed ones, per mode in the order given; every line names
    the BP kernels its decode launched and, where the tree has it, the float32 route.  Then, per code, the rows whose decisions or flags differ
    between the first mode and every other one of this call."""
    import torch
    from ldpc_amd.engine import HipBpEngine, launch_log
    for name, h, pri, p, osd in _node_configs():
        h = h.tocsr()
        h.eliminate_zeros()
        h.sort_indices()
        m, n = h.shape
        eng = HipBpEngine(h.indptr, h.indices, n, np.full(n, p) if pri is None else np.clip(pri, 1e-9, 1 - 1e-9), 30, 1, 0.625)
        if osd:
            eng.set_osd(1, 0)
            eng.set_sampler(pri)
            synd = eng.unpack_b8(eng.sample_b8(12345, 0, batch, device="cuda")[0], m).contiguous()
        else:
            synd = eng.gen_bsc_syndromes(12345, p, 0, batch, device="cuda")
        kept = {}
        for mode in modes:
            eng.set_message_dtype("float64" if mode == "float64" else "float32")
            if hasattr(eng, "set_f32_lane_node"):  # (a checkout from before the switch: float32 is its per-pass route)
                eng.set_f32_lane_node(mode == "float32_lane_node")
            elif mode == "float32_lane_node":
                continue
            route = eng.f32_route(batch, False) if mode != "float64" and hasattr(eng, "f32_route") else None
            out, rates, kms, kernels = None, [], [], None
            for r in range(reps + warmup):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if r == 0:
                    with launch_log() as log:
                        out = eng.decode_batch(synd, want_llr=False, out=out, osd=osd)
                        torch.cuda.synchronize()
                    kernels = {k: v for k, v in sorted(log.items()) if k.startswith("bp_")}
                else:
                    out = eng.decode_batch(synd, want_llr=False, out=out, osd=osd)
                torch.cuda.synchronize()
                if r >= warmup:
                    rates.append(batch / (time.perf_counter() - t0))
                    kms.append(eng.last_kernel_ms())
            kept.setdefault(mode, (out[0].clone(), out[3].clone()))
            print(json.dumps(dict(kind="speed_node", config=name, shape=[m, n], mode=mode, f32_route=route, tree=tree_name or os.path.relpath(_TREE), tag=tag, batch=batch,
                                  osd0=osd, bp_kernels=kernels, syndromes_per_s=[round(x) for x in rates], median_syndromes_per_s=round(float(np.median(rates))),
                                  min_syndromes_per_s=round(min(rates)), max_syndromes_per_s=round(max(rates)), kernel_ms=[round(x, 3) for x in kms],
                                  converged=int(out[3].sum()), mean_iterations=round(float(out[2].double().mean()), 3))), flush=True)
        first = next(iter(kept), None)
        for mode, (dec, cv) in kept.items():
            if mode != first:
                d, c = (dec != kept[first][0]).any(dim=1), cv != kept[first][1]
                print(json.dumps(dict(kind="agreement_node", config=name, batch=batch, modes=[first, mode], tree=tree_name or os.path.relpath(_TREE), tag=tag, osd0=osd,
                                      rows_decisions_differ=int(d.sum()), rows_converge_differ=int(c.sum()), rows_either_differ=int((d | c).sum()))), flush=True)
        del kept
        eng.close()


def agreement(batch):
    import torch
    for name, h, p, osd in _configs(("ldpc36", "bb144")):
        eng = _engine(h, p, 50)
        if osd:
            eng.set_osd(1, 0)
        synd = eng.gen_bsc_syndromes(12345, p, 0, batch, device="cuda")
        res = {}
        for mode in ("float64", "float32"):
            eng.set_message_dtype(mode)
            dec, _, it, cv = eng.decode_batch(synd, want_llr=False, osd=osd)
            torch.cuda.synchronize()
            res[mode] = (dec.clone(), cv.clone(), it.clone())
        d = (res["float64"][0] != res["float32"][0]).any(dim=1)
        c = res["float64"][1] != res["float32"][1]
        i = res["float64"][2] != res["float32"][2]
        print(json.dumps(dict(kind="agreement", config=name, batch=batch, rows_decisions_differ=int(d.sum()), rows_converge_differ=int(c.sum()),
                              rows_either_differ=int((d | c).sum()), share_either_differ=float((d | c).sum()) / batch,
                              rows_iterations_differ=int(i.sum()),
                              converged_float64=int(res["float64"][1].sum()), converged_float32=int(res["float32"][1].sum()))), flush=True)
        eng.close()


def agreement_two_pass(batch, repack):
    """float32 with the two-pass decode (``repack``: -1 = steered by the histogram the decodes before it left, k = forced) against float32
    with set_repack(0), on the configurations and at the size of ``--speed``: rows whose decisions, flags, iteration counts or log-ratio
    BITS differ -- the two must be the same decode."""
    import torch
    from ldpc_amd.engine import launch_log
    for name, h, p, _ in _configs(("ldpc36", "irregular")):
        eng = _engine(h, p, 50)
        eng.set_message_dtype("float32")
        synd = eng.gen_bsc_syndromes(12345, p, 0, batch, device="cuda")
        res = {}
        for tag, k in (("plain", 0), ("two_pass", repack)):
            eng.set_repack(k)
            out = None
            for r in range(3):  # (the first decode on a handle leaves the histogram, the third is certainly steered by one)
                with launch_log() as log:
                    out = eng.decode_batch(synd, want_llr=True, out=out)
                    torch.cuda.synchronize()
            res[tag] = out
            res[tag + "_kernels"] = {k_: v for k_, v in sorted(log.items()) if k_.startswith("bp_")}
        if "bp_f32_gather_lanes_kernel" not in res["two_pass_kernels"] or "bp_f32_gather_lanes_kernel" in res["plain_kernels"]:
            # not a two-pass decode against a plain one (the histogram said "plain", as where nothing converges, or a tree without the two-pass decode): no counts to report
            print(json.dumps(dict(kind="agreement_two_pass", config=name, batch=batch, repack=repack, two_pass_ran=False,
                                  bp_kernels_plain=res["plain_kernels"], bp_kernels_two_pass=res["two_pass_kernels"])), flush=True)
            del res
            eng.close()
            continue
        a, b = res["plain"], res["two_pass"]
        d = (a[0] != b[0]).any(dim=1)
        l = (a[1].view(torch.int64) != b[1].view(torch.int64)).any(dim=1)
        i, c = a[2] != b[2], a[3] != b[3]
        print(json.dumps(dict(kind="agreement_two_pass", config=name, batch=batch, repack=repack, two_pass_ran=True, rows_decisions_differ=int(d.sum()), rows_llr_bits_differ=int(l.sum()),
                              rows_iterations_differ=int(i.sum()), rows_converge_differ=int(c.sum()), rows_any_differ=int((d | l | i | c).sum()),
                              converged=int(a[3].sum()), bp_kernels_plain=res["plain_kernels"], bp_kernels_two_pass=res["two_pass_kernels"])), flush=True)
        del res, a, b
        eng.close()


def speed(batch, modes, reps, repack=-1, tag="", tree_name=None, configs=("ldpc36", "irregular")):
    import torch
    try:
        from ldpc_amd.engine import launch_log as _launch_log
    except ImportError:  # (a checkout from before the launch log)
        _launch_log = None
    for name, h, p, _ in _configs(configs):
        eng = _engine(h, p, 50)
        eng.set_repack(repack)
        synd = eng.gen_bsc_syndromes(12345, p, 0, batch, device="cuda")
        tiles = (batch + 63) // 64
        for mode in modes:
            if mode != "float64" or hasattr(eng, "set_message_dtype"):  # (a checkout from before the mode has float64 only)
                eng.set_message_dtype(mode)
            out = None
            rates, kms = [], []
            kernels = None
            # three untimed: allocations; the first decode on a handle always runs plain and only leaves the histogram that steers the
            # two-pass decode; the third is steered like the timed ones and is the one whose BP kernels are put on record
            for r in range(reps + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if r == 2 and _launch_log is not None:
                    with _launch_log() as log:
                        out = eng.decode_batch(synd, want_llr=False, out=out)
                        torch.cuda.synchronize()
                    kernels = {k: v for k, v in sorted(log.items()) if k.startswith("bp_")}
                else:
                    out = eng.decode_batch(synd, want_llr=False, out=out)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if r >= 3:
                    rates.append(batch / dt)
                    kms.append(eng.last_kernel_ms())
            it = out[2].cpu().numpy().astype(np.int64)
            pad = np.zeros(tiles * 64, np.int64)
            pad[:batch] = it
            tile_iters = int(pad.reshape(tiles, 64).max(axis=1).sum())
            esize = 4 if mode == "float32" else 8
            # what a tile-by-tile flooding decode has to move: 4 message-array passes per tile-iteration (float64: as if nothing were compacted)
            gbytes = tile_iters * 4 * eng.nnz * 64 * esize / 1e9
            _, probe = eng.copy_probe(min(tiles, 1024), eng.nnz, 4)
            print(json.dumps(dict(kind="speed", config=name, mode=mode, tree=tree_name or os.path.relpath(_TREE), tag=tag, repack=repack, batch=batch, bp_kernels=kernels,
                                  syndromes_per_s=[round(x) for x in rates], median_syndromes_per_s=round(float(np.median(rates))),
                                  kernel_ms=[round(x, 2) for x in kms], tile_iterations=tile_iters, message_gbytes=round(gbytes, 1),
                                  message_gbytes_per_s=round(gbytes / (float(np.median(kms)) * 1e-3), 1), copy_probe_gbytes_per_s=round(probe, 1),
                                  fraction_of_copy_probe=round(gbytes / (float(np.median(kms)) * 1e-3) / probe, 3),
                                  converged=int(out[3].sum()))), flush=True)
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--agreement", action="store_true")
    ap.add_argument("--speed", action="store_true")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", default="float64,float32")
    ap.add_argument("--tree", default=None, help="another built checkout to take ldpc_amd from (default: this one)")
    ap.add_argument("--configs", default="large", choices=["large", "small", "node"],
                    help="--speed: the n = 10 000 codes, the small codes of the lane = edge kernels, or the codes beyond them that the lane = node kernels take")
    ap.add_argument("--warmup", type=int, default=3, help="--configs small: untimed decodes before the timed ones")
    ap.add_argument("--tag", default="", help="--speed: copied into every line (which leg of a comparison this is)")
    ap.add_argument("--tree-name", default=None, help="--speed: what the lines call the tree (default: its path)")
    ap.add_argument("--repack", type=int, default=-1, help="--speed (large), --agreement-two-pass: set_repack -- -1 the previous decode's histogram decides (default), 0 off, k a forced first pass")
    ap.add_argument("--only", default="ldpc36,irregular", help="--speed (large): which of the code families to run")
    ap.add_argument("--agreement-two-pass", action="store_true")
    a = ap.parse_args()
    if a.agreement:
        agreement(a.batch)
    if a.agreement_two_pass:
        agreement_two_pass(a.batch, a.repack)
    if a.speed and a.configs == "small":
        speed_small(a.modes.split(","), a.reps, a.warmup, a.tag, a.tree_name)
    elif a.speed and a.configs == "node":
        speed_node(a.batch, a.modes.split(","), a.reps, a.warmup, a.tag, a.tree_name)
    elif a.speed:
        speed(a.batch, a.modes.split(","), a.reps, a.repack, a.tag, a.tree_name, tuple(a.only.split(",")))


if __name__ == "__main__":
    main()
