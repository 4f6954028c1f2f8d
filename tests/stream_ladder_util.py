"""Shared by tests/test_stream_ladder_cases.py (CPU) and tests/test_gpu_stream_instantiations.py (GPU): the case tables that name, for every
selectable instantiation of the STREAMED kernel (bp_decode_kernel), the PER-PASS kernels (bp_spread_*), the on-chip serial_relative kernel
(bp_relative_lds_kernel), the other serial families (bp_serial_kernel, bp_serial_level_kernel, bp_serial_stream_kernel, bp_serial_stream_var_kernel,
bp_serial_lane_kernel, bp_serial_lane_var_kernel, bp_serial_relative_kernel) and the slot kernel (bp_small_kernel), a smallest code that selects it,
for the three METHOD / MATH pairs the library compiles: product-sum exact (0, 0), product-sum with fast math (0, 1), min-sum (1, 0).  The
wavefront ladders of tests/ladder_util.py come once more with fast math.  The expected kernel names are written out here from the size rules of
ldpc_amd/csrc -- tu_stream.hip (pick_kernel, pick_spread_m), host_stream.h (plan_stream, stream_rounds), host_serial.h (pick_serial,
pick_serial_level, plan_serial_stream, decode_serial_streamed, decode_serial_relative_lds: LDPC_PICK_REL), host_onchip.h (decode_onchip) --
nothing is imported from the library but the code builders of ldpc_amd.codes.

Inputs are the ladder's (tests/ladder_util.py): 131 syndromes, max_iter 8, row 0 all zero, one syndrome byte 2 (row 5) and one 3 (row 6), per-column
priors with one p = 0.5 and one p = 0.7 where a case is not uniform; a row-prior case (rp) decodes every row with its own probabilities.
Fast-math cases keep every row at three entries or more: a weight-1 column under a weight-2 check has an exact posterior of exactly 0.0, which only
bit-identical math reproduces (KNIFE_EDGE in tests/test_device_math.py)."""
import ctypes as C
import functools
import os
import subprocess
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import ladder_util as lu
from ladder_util import BATCH, BAD_ROWS, MAX_ITER, build_member

PAIRS = (("product_sum", 0), ("product_sum", 1), ("minimum_sum", 0))  # (method, MATH): what with_method_math (host_handle.h) can name
_M = {"product_sum": 0, "minimum_sum": 1}
_TAG = {("product_sum", 0): "ps", ("product_sum", 1): "psfast", ("minimum_sum", 0): "ms"}

# launches: instantiation -> launches the log must show (None: at least one); the log must show NO other instantiation of FAMILY_KERNELS
# schedule: "parallel" | "serial" | "serial_relative";  mode: set_small_code_kernel;  handoff / ring / serial_kernel / repack: the setter's value (None: not called)
# build: keywords of build_member, or regular: (n, dv, dc, seed) of codes.regular_ldpc_code;  rp: decode_batch(..., channel_probs=P)
# cross: "per_pass" -- the same decode on the per-pass kernels must give the same bits; "rel0" -- the per-lane serial_relative kernel must
SCase = namedtuple("SCase", "id family launches method alpha math schedule mode handoff ring serial_kernel repack switches uniform p seed build regular rp cross")
SCase.__new__.__defaults__ = (None,) * len(SCase._fields)

# every kernel that decodes BP, or prepares a decode kernel's first iteration, in the families walked here and in tests/ladder_util.py
FAMILY_KERNELS = lu.BP_DECODE_KERNELS + (
    "bp_edge0_kernel", "bp_relative_lds_kernel", "bp_serial_relative_kernel", "bp_serial_kernel", "bp_serial_level_kernel", "bp_serial_stream_kernel",
    "bp_serial_stream_var_kernel", "bp_serial_lane_kernel", "bp_serial_lane_var_kernel", "serial_edge0_kernel", "serial_var_init_kernel")


def _b(x):
    return "true" if x else "false"


# ---- the size rules, restated ---------------------------------------------------------------------------------------------------------------
RING_VAR = 9  # LDPC_RING_VAR (bp_stream_kernel.h)


def decode_kernel(method, math, max_row, max_col, ring=0, regular=False, var_ring=False):
    """tu_stream.hip: pick_kernel, with plan_stream's `ring = regular ? ring_depth : 0`.  -> (name, ring depth of the variant)."""
    M, F = _M[method], math
    name = lambda dr, dc, r: f"bp_decode_kernel<{M}, {F}, {dr}, {dc}, {r}>"
    ring = ring if regular else 0
    if var_ring:
        return name(16, 8, RING_VAR), 0
    if ring == 2 and (max_row, max_col) == (6, 3):
        return name(6, 3, 2), 2
    if ring >= 3 and (max_row, max_col) == (6, 3):
        return name(6, 3, 3), 3
    if ring >= (3 if M == 0 else 2) and (max_row, max_col) == (8, 4):
        return name(8, 4, 3), 3
    if M == 0 and ring >= 2 and (max_row, max_col) in ((4, 3), (5, 3)):
        return name(max_row, 3, 2), 2
    for dr, dc in ((4, 3), (6, 3), (8, 4), (8, 8)):
        if max_row <= dr and max_col <= dc:
            return name(dr, dc, 0), 0
    return (name(16, 8, 0) if max_col <= 8 else name(16, 16, 0)), 0


def spread_kernels(method, math, max_row, max_col, nt, rp=False, loop=False):
    """tu_stream.hip: pick_spread_m; host_stream.h: pick_spread, stream_start_per_pass, stream_rounds.  -> dict of the five names."""
    M, F = _M[method], math
    return dict(check=f"bp_spread_check_kernel<{M}, {F}, {8 if max_row <= 8 else 16}, {int(nt)}, {_b(loop)}>",
                bit=f"bp_spread_bit_kernel<{M}, {F}, {4 if max_col <= 4 else 8}, {int(nt)}, {_b(loop)}, {_b(rp)}>",
                init=f"bp_spread_init_kernel<{M}, {F}, {_b(rp)}>", synd=f"bp_spread_synd_kernel<{_b(loop)}>",
                finish=f"bp_spread_finish_kernel<{_b(loop)}, {_b(rp)}>")


def per_pass_launches(method, math, max_row, max_col, nt=0, rp=False):
    """A per-pass start of max_iter rounds: tile 0 holds the two rows that never converge, so every round is queued (stream_rounds)."""
    k = spread_kernels(method, math, max_row, max_col, nt, rp)
    return {k["init"]: 1, k["check"]: MAX_ITER, k["bit"]: MAX_ITER, k["synd"]: MAX_ITER, k["finish"]: MAX_ITER}


def rel_kernel(method, math, max_row, max_col, gs=64, ext=0):
    """host_serial.h: LDPC_PICK_REL.  GS = 16: one table width (8); EXT = 1: rows of 5 .. 16 and columns of 3 .. 8 entries."""
    M, F = _M[method], math
    if ext:
        assert max_row > 4 and max_col > 2
        return f"bp_relative_lds_kernel<{M}, {F}, {8 if max_row <= 8 else 16}, 64, {4 if max_col <= 4 else 8}, 1>"
    dr = 4 if max_row <= 4 else 8 if max_row <= 8 else 16
    dc = 8 if gs == 16 else 2 if max_col <= 2 else 4 if max_col <= 4 else 8
    return f"bp_relative_lds_kernel<{M}, {F}, {dr}, {gs}, {dc}, 0>"


def rel_lds_fits(m, n, nnz, dc, product_sum, gs):
    """host_serial.h: decode_serial_relative_lds keeps the form REL_LDS names only where its state fits: four wavefronts (GS = 16) or one (64)
    beside the shared tables (bp_relative_lds_kernel.h: rel_lds_shared, rel_lds_per_syndrome, rel_lds_scratch), everything in LDS."""
    up = lambda b, a: (b + a - 1) // a * a
    shared = up(n * 8 + (n * 8 if product_sum else 0) + n * dc * 8 + (256 * 8 if product_sum else 0) + up((m + 1) * 2 + nnz * 2 + n, 16), 16)
    per_syn = up(nnz * 8 + n * 8 + up(n * 2, 8) + up(n, 8) + up(m, 8), 16)
    scratch = up(max(2 * n * 4 + up((n + 1) * 2, 8) + up(n, 8), n * 6 + 4 + (n + 2) * 2), 16)
    lds = 160 * 1024 - 64
    no_ext = shared + 4 * (per_syn + scratch) <= lds
    return no_ext and shared + (1 if gs == 64 else 4) * ((64 // gs) * per_syn + scratch) <= lds


def serial_rung(max_row, max_col):
    """host_serial.h: pick_serial / pick_serial_level -- <DC, DR> of the instantiation."""
    return "2, 4" if max_row <= 4 and max_col <= 2 else "3, 6" if max_row <= 6 and max_col <= 3 else "4, 8"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def _shape(dr, dc, n=150, min_row=1):
    """m rows for about n columns, as the wavefront ladders of ladder_util size theirs -- fewer where the rows' entries would fill the columns
    beyond 0.7 of their bound: the builder needs room for its one heaviest column and for columns of one entry."""
    m = min(n * (1 + dc) / (1 + dr), 0.6 * n)  # (at most 0.6 n checks: a code with more of them converges on every row at any noise)
    fill = (1 + dc) * (min_row + dr) / (2 * (1 + dr)) / (0.7 * dc)
    return dict(m=max(round(m / max(fill, 1.0)), dc), max_row=dr, max_col=dc, min_row=min_row, n=n)


def _p(dr, dc):
    """The noise at which the oracle converges on some of a shape's 131 rows and not on others (tests/test_stream_ladder_cases.py): codes with
    columns of two entries at most, or rows of four at most under heavier columns, are weak; the others take more."""
    return 0.01 if dc <= 2 or dr >= 32 else 0.015 if dr <= 4 and dc >= 4 else 0.03 if dc <= 3 or (dr >= 16 and dc <= 4) else 0.06


def _min_row(math, dr):
    return min(3, dr) if math else 1  # (fast math: no weight-2 check, see the module's docstring)


# both ends of every register rung of pick_kernel: the lightest code a rung takes that the rung before does not, and the rung's bound;
# 17 x 9: beyond every register bound -- "heavier nodes take the streaming path inside"
DECODE_RUNGS = (((4, 3), (3, 2), (4, 3)), ((6, 3), (5, 2), (6, 3)), ((8, 4), (4, 4), (8, 4)), ((8, 8), (4, 5), (8, 8)), ((16, 8), (9, 2), (16, 8)),
                ((16, 16), (4, 9), (17, 9)))
# regular codes of the ring variants: (row weight, column weight) -> (n, dv, dc, seed)
REGULAR = {(6, 3): (150, 3, 6, 3), (8, 4): (152, 4, 8, 3), (4, 3): (152, 3, 4, 3), (5, 3): (150, 3, 5, 3)}


def _decode_cases():
    out = []
    for method, math in PAIRS:
        tag, alpha = _TAG[(method, math)], 0.625 if method == "minimum_sum" else 1.0
        mk = lambda id, launches, seed, **kw: SCase(id=f"decode-{tag}-{id}", family="decode", launches=launches, method=method, alpha=alpha, math=math,
                                                    schedule="parallel", mode=0, handoff=0, seed=seed, cross=None if math else "per_pass",
                                                    **{"switches": {}, **kw})
        for k, (rung, low, high) in enumerate(DECODE_RUNGS):
            for end, (dr, dc) in (("low", low), ("high", high)):
                name, _ = decode_kernel(method, math, dr, dc)
                assert name == f"bp_decode_kernel<{_M[method]}, {math}, {rung[0]}, {rung[1]}, 0>"
                out.append(mk(f"{rung[0]}x{rung[1]}-{end}-{dr}x{dc}", {name: 1}, 9000 + 100 * k + 10 * (end == "high") + math, uniform=(dr + k) % 2 == 0,
                              p=_p(dr, dc), build=_shape(dr, dc, min_row=_min_row(math, dr))))
        for (dr, dc), depth in (((6, 3), 2), ((6, 3), 3), ((8, 4), 3), ((8, 4), 2), ((4, 3), 2), ((5, 3), 2)):
            name, ring = decode_kernel(method, math, dr, dc, ring=depth, regular=True)
            launches = {name: 1}
            if ring:  # stream_persistent: the first check pass of a ring variant reads the table bp_edge0_kernel leaves
                launches[f"bp_edge0_kernel<{_M[method]}, {math}>"] = 1
            out.append(mk(f"ring{depth}-{dr}x{dc}", launches, 9700 + 10 * dr + depth, ring=depth, regular=REGULAR[(dr, dc)], uniform=depth == 2,
                          p={(6, 3): 0.05, (8, 4): 0.06, (4, 3): 0.12, (5, 3): 0.07}[(dr, dc)]))
        name, _ = decode_kernel(method, math, 16, 8, var_ring=True)
        out.append(mk("var_ring-12x7", {name: 1}, 9800 + math, switches={"VAR_RING": 1}, uniform=False, p=_p(12, 7), build=_shape(12, 7, min_row=_min_row(math, 12))))
    return out


# compiled, but no rule of pick_kernel selects them (the (3,4)- and (3,5)-regular rings are product-sum only): id of the case that shows
# what runs instead -> (the instantiation, the reason)
NOT_SELECTABLE = {
    "decode-ms-ring2-4x3": ("bp_decode_kernel<1, 0, 4, 3, 2>", "pick_kernel: the (3,4)-regular ring is product-sum only; min-sum at ring 2 runs <1, 0, 4, 3, 0>"),
    "decode-ms-ring2-5x3": ("bp_decode_kernel<1, 0, 5, 3, 2>", "pick_kernel: the (3,5)-regular ring is product-sum only; min-sum at ring 2 runs <1, 0, 6, 3, 0>"),
}


def _spread_cases():
    """A per-pass start (hand-off threshold above the 3 tiles; one product-sum case by the automatic rule): DR <= 8 and 9 .. 16, DC <= 4 and
    5 .. 8, both cache policies (SPREAD_NT), shared and row priors, 1 / 4 / 16 nodes per wavefront (SPREAD_NODES; 1 is what 3 tiles get)."""
    out = []
    for method, math in PAIRS:
        tag, alpha = _TAG[(method, math)], 0.625 if method == "minimum_sum" else 1.0
        # (DR, DC, NT, RP, SPREAD_NODES): every (DR, NT) of the check kernel and every (DC, NT, RP) of the bit kernel, each DR with each DC
        for k, (dr, dc, nt, rp, nodes) in enumerate(((8, 4, 0, False, None), (16, 4, 0, True, 4), (16, 4, 1, False, 16), (8, 4, 1, True, None),
                                                     (16, 8, 0, False, 16), (8, 8, 0, True, None), (8, 8, 1, False, 4), (16, 8, 1, True, None))):
            # shared priors: AT the bounds; row priors: the far end of the rung -- rows of 5 and of 9, columns of 3 and of 5 entries
            rows, cols = ({8: 5, 16: 9}[dr], {4: 3, 8: 5}[dc]) if rp else (dr, dc)
            switches = {"SPREAD_NT": nt, **({"SPREAD_NODES": nodes} if nodes else {})}
            auto = method == "product_sum" and k == 0  # plan_stream: per_pass_first
            out.append(SCase(id=f"spread-{tag}-{rows}x{cols}-nt{nt}-{'rp' if rp else 'shared'}-nodes{nodes or 1}", family="spread",
                             launches=per_pass_launches(method, math, rows, cols, nt, rp), method=method, alpha=alpha, math=math, schedule="parallel", mode=0,
                             handoff=None if auto else 1000, switches=switches, uniform=k % 2 == 0, p=_p(rows, cols), seed=10000 + 100 * _M[method] + 10 * k + math,
                             build=_shape(rows, cols, min_row=_min_row(math, rows)), rp=rp))
    return out


REL_SHAPES = ((4, 2), (4, 4), (4, 8), (8, 2), (8, 4), (8, 8), (16, 2), (16, 4), (16, 8))  # DR by the heaviest row, DC by the heaviest column: each AT its bound
REL_N = 100


def _rel_cases():
    out = []
    for method, math in PAIRS:
        tag, alpha = _TAG[(method, math)], 0.625 if method == "minimum_sum" else 1.0
        for k, (dr, dc) in enumerate(REL_SHAPES):
            forms = [("gs64", 64, 0, {"REL_LDS": 64})]
            if dc == 8:
                forms.append(("gs16", 16, 0, {"REL_LDS": 16}))
            if dr > 4 and dc > 2:
                forms.append(("ext", 64, 1, {"REL_EXT": 1}))
            for form, gs, ext, sw in forms:
                for sweep in (("levels", "walk") if gs == 64 else ("walk",)):  # (GS = 16 implies bit by bit)
                    launches = {rel_kernel(method, math, dr, dc, gs, ext): 1}
                    if ext and method == "product_sum":  # (the edge form of the priors: a table in global memory there)
                        launches[f"serial_edge0_kernel<0, {math}>"] = 1
                    out.append(SCase(id=f"rel-{tag}-{dr}x{dc}-{form}-{sweep}", family="rel", launches=launches, method=method, alpha=alpha, math=math,
                                     schedule="serial_relative", mode=None, switches={**sw, **({"REL_LEVELS": 0} if sweep == "walk" and gs == 64 else {})},
                                     uniform=k % 2 == 0, p=_p(dr, dc), seed=11000 + 10 * k + math, build=_shape(dr, dc, n=REL_N, min_row=_min_row(math, dr)),
                                     cross=None if math else "rel0"))
    return out


def _serial_cases():
    out = []
    for method, math in PAIRS:
        M, tag, alpha = _M[method], _TAG[(method, math)], 0.625 if method == "minimum_sum" else 1.0
        mk = lambda id, launches, seed, **kw: SCase(id=f"serial-{tag}-{id}", family="serial", launches=launches, method=method, alpha=alpha, math=math,
                                                    schedule="serial", **{"switches": {}, "seed": seed + math, **kw})
        # one wavefront walks the bits (set_serial_kernel 0) / a workgroup takes a level (1): rungs (4,2), (6,3), beyond; 12 x 6: heavier nodes are streamed (SerialArgs::fast == 0)
        for k, (dr, dc) in enumerate(((4, 2), (6, 3), (8, 4), (12, 6))):
            for sk, base in ((0, "bp_serial_kernel"), (1, "bp_serial_level_kernel")):
                out.append(mk(f"{'walk' if sk == 0 else 'level'}-{dr}x{dc}", {f"{base}<{M}, {math}, {serial_rung(dr, dc)}>": 1}, 12000 + 10 * k, serial_kernel=sk,
                              uniform=(k + sk) % 2 == 0, p=_p(dr, dc), build=_shape(dr, dc, min_row=_min_row(math, dr))))
        # the streamed forms (set_serial_kernel 2).  131 rows go to the workgroup-per-syndrome kernels from the start (decode_serial_streamed:
        # lane_only) unless the decode is one pass (set_repack 0): then tiles.  (6,3)-regular: bp_serial_stream_kernel<., ., 6, 3, SER_RING>
        for ring in (1, 2):
            out.append(mk(f"stream-ring{ring}", {f"bp_serial_stream_kernel<{M}, {math}, 6, 3, {ring}>": 1, f"serial_edge0_kernel<{M}, {math}>": 1}, 12100 + ring,
                          serial_kernel=2, repack=0, switches={"SER_RING": ring}, uniform=ring == 1, p=0.06, regular=REGULAR[(6, 3)]))
        out.append(mk("lane", {f"bp_serial_lane_kernel<{M}, {math}, 6, 3>": 1}, 12110, serial_kernel=2, uniform=True, p=0.06, regular=REGULAR[(6, 3)]))
        for k, (dr, dc) in enumerate(((8, 4), (16, 8))):  # the item forms: any other degree profile
            out.append(mk(f"stream_var-{dr}x{dc}", {f"bp_serial_stream_var_kernel<{M}, {math}, {dr}, {dc}>": 1, f"serial_var_init_kernel<{M}, {math}>": 1}, 12200 + 10 * k,
                          serial_kernel=2, repack=0, uniform=k == 0, p=_p(dr, dc), build=_shape(dr, dc, min_row=_min_row(math, dr))))
            out.append(mk(f"lane_var-{dr}x{dc}", {f"bp_serial_lane_var_kernel<{M}, {math}, {dr}, {dc}>": 1}, 12300 + 10 * k, serial_kernel=2, uniform=k == 1,
                          p=_p(dr, dc), build=_shape(dr, dc, min_row=_min_row(math, dr))))
        # serial_relative on the per-lane kernel (REL_LDS 0)
        out.append(SCase(id=f"serial-{tag}-relative-per-lane", family="serial", launches={f"bp_serial_relative_kernel<{M}, {math}>": 1}, method=method, alpha=alpha, math=math,
                         schedule="serial_relative", switches={"REL_LDS": 0}, uniform=False, p=_p(8, 4), seed=12400 + math, build=_shape(8, 4, n=REL_N, min_row=_min_row(math, 8))))
        # the slot kernel (set_small_code_kernel 2), shared and row priors
        for rp in (False, True):
            out.append(SCase(id=f"small-{tag}-{'rp' if rp else 'shared'}", family="small", launches={f"bp_small_kernel<{M}, {math}, {_b(rp)}>": None}, method=method, alpha=alpha,
                             math=math, schedule="parallel", mode=2, switches={}, uniform=rp, p=_p(8, 4), seed=12500 + 10 * rp + math, build=_shape(8, 4, min_row=_min_row(math, 8)), rp=rp))
    return out


def _fast_wave_cases():
    """The product-sum WAVE_CASES and every WAVE_PS_CASE of tests/ladder_util.py once more with fast math, on a code of the same shape without weight-2 checks."""
    out = []
    for c in lu.WAVE_CASES + lu.WAVE_PS_CASES:
        if c.method != "product_sum":
            continue
        kernel = c.kernel.replace("bp_wave_kernel<0, 0,", "bp_wave_kernel<0, 1,").replace("bp_wave_ps_kernel<0,", "bp_wave_ps_kernel<1,")
        assert kernel != c.kernel
        out.append(SCase(id=f"fast-{c.id}", family="wave", launches={kernel: 1}, method=c.method, alpha=c.alpha, math=1, schedule="parallel", mode=c.mode,
                         switches=dict(c.switches), uniform=c.uniform, p=_p(c.build["max_row"], c.build["max_col"]), seed=c.seed + 5, build=_shape(c.build["max_row"], c.build["max_col"], min_row=_min_row(1, c.build["max_row"]))))
    return out


DECODE_CASES = _decode_cases()
SPREAD_CASES = _spread_cases()
REL_CASES = _rel_cases()
SERIAL_CASES = _serial_cases()
FAST_WAVE_CASES = _fast_wave_cases()
ALL_CASES = DECODE_CASES + SPREAD_CASES + REL_CASES + SERIAL_CASES + FAST_WAVE_CASES
BY_ID = {c.id: c for c in ALL_CASES}

# The templates walked here and in the LOOP cases below: every compiled instantiation of them must be some case's launch or in NOT_SELECTABLE
WALKED_TEMPLATES = ("bp_decode_kernel", "bp_spread_check_kernel", "bp_spread_bit_kernel", "bp_spread_init_kernel", "bp_spread_finish_kernel", "bp_spread_synd_kernel",
                    "bp_edge0_kernel", "bp_relative_lds_kernel", "bp_serial_relative_kernel", "bp_serial_kernel", "bp_serial_level_kernel", "bp_serial_stream_kernel",
                    "bp_serial_stream_var_kernel", "bp_serial_lane_kernel", "bp_serial_lane_var_kernel", "serial_edge0_kernel", "serial_var_init_kernel", "bp_small_kernel")

# ---- the LOOP forms of the per-pass kernels ------------------------------------------------------------------------------------------------------
# A second pass whose list of tiles, compacted after its eighth round, is LONGER than 32: slots 32 .. are the looping forms' (stream_rounds).
# An easy batch (all-zero syndromes, which converge in their first iteration, and LOOP_EASY_HOPELESS rows that never do) leaves the histogram that
# makes the next decode on the handle compact (late_rows <= 24, grid above 40 tiles); the hard batch
# holds LOOP_HOPELESS rows with a syndrome byte 2, which never converge: they alone fill 47 tiles after the lane compaction, so at least 15 tiles lie
# beyond slot 32 and the 8 workgroup rows of a looping launch take more than one each.
LoopCase = namedtuple("LoopCase", "id method alpha math nt build seed")
LOOP_BATCH = 4096 + 37     # 65 tiles, the last one partial
LOOP_HOPELESS = 3000
LOOP_EASY_HOPELESS = 10
LOOP_MAX_ITER = 24
LOOP_P = 0.02
LOOP_CASES = [LoopCase(id=f"loop-{_TAG[(method, math)]}-{dr}x{dc}-nt{nt}", method=method, alpha=0.625 if method == "minimum_sum" else 1.0, math=math, nt=nt,
                       build=_shape(dr, dc, min_row=_min_row(math, dr)), seed=13000 + 100 * _M[method] + 10 * nt + math + dr)
              for method, math in PAIRS for (dr, dc), nt in (((8, 4), 0), ((16, 8), 1), ((8, 4), 1), ((16, 8), 0))]


LOOP_SAMPLE = np.r_[0:48, LOOP_BATCH - 16:LOOP_BATCH]  # rows of the hard batch that are checked against the oracle


def loop_launches(c):
    """What the log of the steered decode of the hard batch must hold of the per-pass families: the plain and the looping form of each kernel."""
    out = set()
    for loop in (False, True):
        k = spread_kernels(c.method, c.math, c.build["max_row"], c.build["max_col"], c.nt, False, loop)
        out |= {k["check"], k["bit"], k["synd"], k["finish"]}
    return out


@functools.lru_cache(maxsize=None)
def loop_expected(case_id, fast=False):
    """The oracle's results on LOOP_SAMPLE of the hard batch."""
    import oracle
    c = next(c for c in LOOP_CASES if c.id == case_id)
    h, _, hard, _ = loop_inputs(case_id)
    o = oracle.BpOracle(h, error_rate=LOOP_P, max_iter=LOOP_MAX_ITER, bp_method=c.method, ms_scaling_factor=c.alpha)
    if fast:
        plug_fast_math(o)
    with np.errstate(all="ignore"):
        return o.decode_batch(hard[LOOP_SAMPLE])


@functools.lru_cache(maxsize=None)
def loop_inputs(case_id):
    """(h, easy syndromes, hard syndromes, hopeless rows of the hard batch)."""
    c = next(c for c in LOOP_CASES if c.id == case_id)
    h = build_member(c.seed, **c.build)
    m, n = h.shape
    rng = np.random.default_rng(c.seed + 1)

    def draw(p):
        e = (rng.random((LOOP_BATCH, n)) < p).astype(np.uint8)
        return np.ascontiguousarray((h @ e.T % 2).T.astype(np.uint8))

    easy, hard = np.zeros((LOOP_BATCH, m), np.uint8), draw(LOOP_P)  # (easy: every row converges in its first iteration, but the few below)
    easy[rng.choice(LOOP_BATCH, size=LOOP_EASY_HOPELESS, replace=False), 0] = 2
    hopeless = np.sort(rng.choice(LOOP_BATCH, size=LOOP_HOPELESS, replace=False))
    hard[hopeless, rng.integers(m, size=LOOP_HOPELESS)] = 2
    for x in (easy, hard, hopeless):
        x.setflags(write=False)
    return h, easy, hard, hopeless


# ---- inputs and oracles ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix(case_id):
    c = BY_ID[case_id]
    if c.regular:
        from ldpc_amd import codes
        n, dv, dc, seed = c.regular
        return sp.csr_matrix(codes.regular_ldpc_code(n, dv, dc, seed=seed))
    return build_member(c.seed, **c.build)


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """(h, probs, syndromes, row probabilities or None) of a case: built once, shared (treat as read-only).  As ladder_util.inputs."""
    c = BY_ID[case_id]
    h = matrix(case_id)
    m, n = h.shape
    rng = np.random.default_rng(c.seed + 1)
    if c.uniform:
        probs = np.full(n, c.p)
    else:
        probs = rng.uniform(0.01, 0.15, size=n)
        a, b = (int(x) for x in rng.choice(n, size=2, replace=False))
        probs[a], probs[b] = 0.5, 0.7
    e = (rng.random((BATCH, n)) < c.p).astype(np.uint8)
    synd = np.ascontiguousarray((h @ e.T % 2).T.astype(np.uint8))
    synd[0] = 0
    synd[BAD_ROWS[0], int(rng.integers(m))] = 2
    synd[BAD_ROWS[1], int(rng.integers(m))] = 3
    row_probs = None
    if c.rp:  # every row its own probabilities: the case's, scaled bit by bit by 0.6 .. 1.4; rows 1 and 2 keep a p = 0.5 and a p = 0.7
        row_probs = np.ascontiguousarray(np.clip(np.where(probs < 0.5, probs, c.p) * rng.uniform(0.6, 1.4, size=(BATCH, n)), 1e-6, 0.45))
        row_probs[1, int(rng.integers(n))] = 0.5
        row_probs[2, int(rng.integers(n))] = 0.7
        row_probs.setflags(write=False)
    for x in (probs, synd):
        x.setflags(write=False)
    return h, probs, synd, row_probs


_NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


@functools.lru_cache(maxsize=None)
def device_math():
    """The device's math routines compiled for the host (ldpc_amd/csrc/bp_math.h through tests/native/device_math_host.cpp), as tests/test_device_math.py builds them."""
    src, so = os.path.join(_NATIVE, "device_math_host.cpp"), os.path.join(_NATIVE, "libdevice_math_host.so")
    hdr = os.path.join(os.path.dirname(_NATIVE), os.pardir, "ldpc_amd", "csrc", "bp_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        tmp = f"{so}.{os.getpid()}.tmp"  # (built aside and moved into place: another test process may be loading or building it)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    for f in ("dm_tanh_half_ptr", "dm_log_ratio_ptr"):
        getattr(lib, f).restype = C.c_void_p
    return lib


def plug_fast_math(o):
    """oracle/bp_oracle.c: bp_oracle_set_math -- the parallel loop and every serial schedule's product-sum site honour the substitutes."""
    dm = device_math()
    o.lib.bp_oracle_set_math.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    o.lib.bp_oracle_set_math(o._h, dm.dm_tanh_half_ptr(), dm.dm_log_ratio_ptr())
    return o


def _run_oracle(case_id, fast):
    import oracle
    c = BY_ID[case_id]
    h, probs, synd, row_probs = inputs(case_id)
    o = oracle.BpOracle(h, error_channel=probs, max_iter=MAX_ITER, bp_method=c.method, ms_scaling_factor=c.alpha)
    if fast:
        plug_fast_math(o)
    with np.errstate(all="ignore"):
        if c.schedule == "serial":
            return o.decode_serial_batch(synd, None)
        if c.schedule == "serial_relative":
            return o.decode_serial_relative_batch(synd, fresh=True)  # (..., the order the last row leaves)
        if row_probs is None:
            return o.decode_batch(synd)
        dec, llr, it, cv = np.zeros((BATCH, h.shape[1]), np.uint8), np.zeros((BATCH, h.shape[1])), np.zeros(BATCH, np.int32), np.zeros(BATCH, bool)
        for b in range(BATCH):  # the reference's loop: update_channel_probs(P[b]); decode(S[b])
            o.channel_probs = np.ascontiguousarray(row_probs[b])
            d, l, i, v = o.decode_batch(synd[b:b + 1])
            dec[b], llr[b], it[b], cv[b] = d[0], l[0], i[0], v[0]
        return dec, llr, it, cv


@functools.lru_cache(maxsize=None)
def expected(case_id):
    """The exact oracle's (decoding, llr, iterations, converge[, final order]) of a case: computed once."""
    return _run_oracle(case_id, False)


@functools.lru_cache(maxsize=None)
def expected_fast(case_id):
    """The oracle with the device's fast routines plugged in: what a fast-math kernel is predicted to compute."""
    assert BY_ID[case_id].math == 1
    return _run_oracle(case_id, True)
