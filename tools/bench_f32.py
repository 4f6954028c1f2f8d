#!/usr/bin/env python
"""float32 message mode against float64: agreement of the results, and speed.

    python tools/bench_f32.py --agreement                 # share of rows whose decisions / converge flags differ between the modes
    python tools/bench_f32.py --speed                     # syndromes/s of both modes + the copy probe, same process, same box
    python tools/bench_f32.py --speed --modes float64 --tree <checkout>   # the float64 of another built checkout (the parent commit: A/B on one box)
    python tools/bench_f32.py --speed --configs small     # the small codes the on-chip kernels take (each at its own batch sizes)
    python tools/bench_f32.py --speed --repack 0          # ... with the two-pass decode off (set_repack; default -1: the previous decode's histogram decides)
    python tools/bench_f32.py --agreement-two-pass        # float32 two-pass against float32 with set_repack(0): rows that differ, log-ratio bits included

Configurations: (3,6)-regular n = 10 000, min-sum 50 iterations, at p = 0.05 and 0.09; the irregular n = 10 000 code of
``bench.py --full`` (speed only); BB144 min-sum 50 + OSD-0 (agreement only).  ``--configs small`` (speed only): the codes whose messages
stay on chip in both modes -- BB144 min-sum 50 at p = 0.05 (B = 65 536 and 262 144; bp_edge8, DC 3), the rotated surface code d = 21 min-sum
30 at p = 0.05 (B = 262 144; bp_edge) and the hypergraph product of hamming_code(3) with itself min-sum 30 at p = 0.05 (B = 262 144;
bp_edge8, DC 4); every line names the BP kernels its decode launched (``bp_kernels``, from the launch log), so the route is on record.
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
    ap.add_argument("--configs", default="large", choices=["large", "small"], help="--speed: the n = 10 000 codes, or the small codes of the on-chip kernels")
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
    elif a.speed:
        speed(a.batch, a.modes.split(","), a.reps, a.repack, a.tag, a.tree_name, tuple(a.only.split(",")))


if __name__ == "__main__":
    main()
