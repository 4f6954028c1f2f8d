"""Shared by tests/test_near_one_cases.py (CPU) and tests/test_gpu_near_one.py (GPU): inputs that drive the near-1 parking of the exact
product-sum `log` to and past its capacity, and a census that says -- without the library -- which of its paths every input reaches.

The exact log has a branch for arguments q = (1 + x) / (1 - x) inside [1 - 2^-4, 1 + 0x1.09p-4) and a table branch for the rest.  Three pieces of
device code evaluate the table branch everywhere, park the near-1 arguments in a small LDS buffer and run the near-1 branch once over it:
  check_row      check_row_ps_exact_fast (bp_device_common.h): bp_decode_kernel, bp_spread_check_kernel; per check row of a 64-syndrome tile,
                 entries visited last to first, LDPC_NEAR_SLOTS arguments
  bit_messages   bit_messages_ps_exact_fast (bp_serial_stream_kernel.h): bp_serial_stream_kernel; per bit of a tile, the bit's checks in order
  wave           check B of bp_wave_ps_kernel without a team (bp_wave_kernel.h): per syndrome and iteration, rounds of 64 entry slots (rows padded
                 to DR), LDPC_PS_NEAR_SLOTS entries
An entry whose lanes do not all fit is evaluated in place.  The first two count LIVE lanes only (a converged syndrome's lane, or a lane past the
end of the batch, is dead) and leave a row / bit to the generic routine when a live lane holds |tanh| = 1 or a NaN (or the row has one entry);
the wave kernel decides per iteration (`tame`).

The census comes from a plain NumPy float64 restatement of flooding and serial product-sum (flood, serial below).  It is not bit-exact and does
not have to be: it only classifies arguments, and arguments within 1e-9 relative of a threshold are set aside and counted as `borderline` (the
CPU test asserts there are none, and none of the tanh arguments is close to where tanh saturates).

How the inputs get there: a degree-1 "pendant" column with p = 0.4999 sends its check tanh(0.0002) for ever, so every OTHER entry of that check has a
near-1 argument in every lane and iteration (a check with two pendants: every entry).  A (3,6)-regular code has no pendant; there a pair of
columns with p just below 0.5 that share their three checks plays the part.  A syndrome byte above 1 keeps a lane live to the last iteration, an
all-zero syndrome makes it dead from iteration 2, lanes past the end of a partial tile are dead from the start: the number of live lanes times
the near-1 entries of a row is what the buffer sees."""
import functools
import os
import re
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import ladder_util as lu

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ldpc_amd", "csrc")
LO, HI = 1.0 - 2.0 ** -4, 1.0 + float.fromhex("0x1.09p-4")  # glibc log's near-1 interval [LO, HI)
GUARD = 1e-9
SATURATION_BAND = (37.5, 38.8)  # tanh(b / 2) rounds to exactly 1 from |b| = 38.13 on: no live argument may come this close


@functools.lru_cache(maxsize=None)
def slot_counts():
    """{"check_row": LDPC_NEAR_SLOTS, "bit_messages": LDPC_NEAR_SLOTS, "wave": LDPC_PS_NEAR_SLOTS}, read from the headers."""
    def define(header, name):
        found = re.findall(rf"^#define {name} (\d+)\b", open(os.path.join(_CSRC, header)).read(), flags=re.M)
        assert len(found) == 1, (header, name, found)
        return int(found[0])
    near = define("bp_device_common.h", "LDPC_NEAR_SLOTS")
    return {"check_row": near, "bit_messages": near, "wave": define("bp_wave_kernel.h", "LDPC_PS_NEAR_SLOTS")}


def labels_of(counts, capacity):
    """What a sequence of per-step near-1 counts (entries of a row, checks of a bit, rounds of a pass) does to a buffer of `capacity`:
    zero | under | at (filled exactly, nothing in place) | over_first (the first step with near-1 arguments does not fit) |
    park_then_over (a step does not fit behind what is parked)."""
    total, over, out = 0, False, set()
    for c in counts:
        if c == 0:
            continue
        if total + c <= capacity:
            total += c
        else:
            out.add("park_then_over" if total else "over_first")
            over = True
    if not over:
        out.add("zero" if total == 0 else "at" if total == capacity else "under")
    return out


def _classify(q):
    border = (np.abs(q / LO - 1.0) < GUARD) | (np.abs(q / HI - 1.0) < GUARD)
    return (q >= LO) & (q < HI) & ~border, border


def _band(b):
    a = np.abs(b)
    return (a > SATURATION_BAND[0]) & (a < SATURATION_BAND[1])


Census = namedtuple("Census", "labels borderline iterations converge detail")


class _Tally:
    def __init__(self, capacity):
        self.capacity, self.labels, self.borderline, self.detail = capacity, set(), 0, []

    def unit(self, it, tile, unit, counts, fallback, dead_near):
        got = {"fallback"} if fallback else labels_of(counts, self.capacity)
        if dead_near and not fallback:
            got.add("dead_near")
        self.labels |= got
        self.detail.append((it, tile, unit, tuple(int(c) for c in counts), tuple(sorted(got))))


def _setup(h, probs, synd):
    h = sp.csr_matrix(h)
    h.sort_indices()
    m, n = h.shape
    batch = len(synd)
    tiles = (batch + 63) // 64
    s = np.zeros((tiles * 64, m), np.uint8)
    s[:batch] = synd
    prior = np.log((1.0 - probs) / probs)
    csc = sp.csr_matrix((np.arange(1, h.nnz + 1), h.indices, h.indptr), shape=h.shape).tocsc()  # data: 1 + the CSR position of each entry
    csc.sort_indices()
    csc.data -= 1
    return h, m, n, batch, tiles, s, prior, csc


def _ratio(x):
    with np.errstate(all="ignore"):
        return (1.0 + x) / (1.0 - x)


def flood(h, probs, synd, max_iter, capacity, wave_dr=None, wave_capacity=None):
    """Flooding product-sum (bp.hpp:192-325) on every lane of every tile, dead lanes included -> (Census of check_row, Census of the wave
    kernel's check B or None).  A dead lane's values count for `dead_near` only in its first dead iteration: there they are what its last live
    bit pass left, whatever a kernel does with dead lanes afterwards."""
    h, m, n, batch, tiles, s, prior, csc = _setup(h, probs, synd)
    rp, ci = h.indptr, h.indices
    lanes = tiles * 64
    bmsg = np.tile(prior[ci], (lanes, 1))  # bit -> check log-ratios, CSR order
    done = np.arange(lanes) >= batch
    died = np.where(done, 0, -1)           # iteration after which a lane is dead
    iters = np.zeros(lanes, np.int32)
    row, wave = _Tally(capacity), _Tally(wave_capacity)
    sign = np.where(s != 0, -1.0, 1.0)
    min_rdeg = int(np.diff(rp).min())
    for it in range(1, max_iter + 1):
        live = ~done
        if not live.any():
            break
        fresh_dead = done & (died == it - 1)
        row.borderline += int((_band(bmsg) & live[:, None]).sum())
        a = np.tanh(bmsg / 2.0)
        wild = ~(np.abs(a) < 1.0)
        c = np.empty_like(bmsg)
        near_all = np.zeros(bmsg.shape, bool)
        for i in range(m):
            rs, d = rp[i], rp[i + 1] - rp[i]
            t = a[:, rs:rs + d]
            x = np.stack([np.prod(np.delete(t, k, axis=1), axis=1) for k in range(d)], axis=1)
            q = _ratio(x)
            near, border = _classify(q)
            near_all[:, rs:rs + d] = near
            with np.errstate(all="ignore"):
                c[:, rs:rs + d] = np.log(q) * sign[:, i:i + 1]
            bad = wild[:, rs:rs + d].any(axis=1)
            for tile in range(tiles):
                sl = slice(64 * tile, 64 * tile + 64)
                lv = live[sl]
                if not lv.any():
                    continue  # (the tile has retired)
                fallback = d < 2 or bool((bad[sl] & lv).any())
                if not fallback:
                    row.borderline += int((border[sl] & lv[:, None]).sum())
                counts = [int((near[sl, k] & lv).sum()) for k in range(d - 1, -1, -1)]
                dead_near = any((near[sl, k] & fresh_dead[sl]).any() and (~near[sl, k] & lv).any() for k in range(d))
                row.unit(it, tile, i, counts, fallback, dead_near)
        if wave_dr is not None:  # one wavefront per syndrome: rounds of 64 slots, row i at slots i DR .. i DR + d - 1
            slot = np.concatenate([i * wave_dr + np.arange(rp[i + 1] - rp[i]) for i in range(m)])
            for b in np.flatnonzero(live[:batch]):
                tame = not wild[b].any() and min_rdeg >= 2
                counts = np.bincount(slot[near_all[b]] // 64, minlength=(m * wave_dr + 63) // 64)
                wave.unit(it, int(b), -1, counts if tame else (), not tame, False)
        llr = np.empty((lanes, n))
        for j in range(n):
            e = csc.data[csc.indptr[j]:csc.indptr[j + 1]]
            cj = c[:, e]
            with np.errstate(all="ignore"):
                llr[:, j] = prior[j] + cj.sum(axis=1)
                for k in range(len(e)):
                    bmsg[:, e[k]] = prior[j] + np.delete(cj, k, axis=1).sum(axis=1)
        hard = (llr <= 0).astype(np.int64)
        ok = ((hard @ h.T.toarray()) % 2 == s).all(axis=1)
        newly = ok & ~done
        iters[live] = it
        died[newly] = it
        done = done | ok
    conv = done[:batch] & (died[:batch] > 0)
    out_row = Census(row.labels, row.borderline, iters[:batch].copy(), conv, row.detail)
    out_wave = Census(wave.labels, row.borderline, iters[:batch].copy(), conv, wave.detail) if wave_dr is not None else None
    return out_row, out_wave


def serial(h, probs, synd, max_iter, capacity):
    """Serial product-sum, bits 0 .. n - 1 (bp.hpp:451-545), on every lane of every tile -> Census of bit_messages (unit = bit)."""
    h, m, n, batch, tiles, s, prior, csc = _setup(h, probs, synd)
    rp = h.indptr
    lanes = tiles * 64
    bmsg = np.tile(prior[h.indices], (lanes, 1))
    done = np.arange(lanes) >= batch
    died = np.where(done, 0, -1)
    iters = np.zeros(lanes, np.int32)
    tally = _Tally(capacity)
    sign = np.where(s != 0, -1.0, 1.0)
    row_of = np.repeat(np.arange(m), np.diff(rp))
    for it in range(1, max_iter + 1):
        live = ~done
        if not live.any():
            break
        fresh_dead = done & (died == it - 1)
        llr = np.empty((lanes, n))
        for j in range(n):
            own = csc.data[csc.indptr[j]:csc.indptr[j + 1]]
            cj = np.empty((lanes, len(own)))
            near = np.zeros((lanes, len(own)), bool)
            border = np.zeros((lanes, len(own)), bool)
            bad = np.zeros(lanes, bool)
            for k, e in enumerate(own):
                i = row_of[e]
                others = [q for q in range(rp[i], rp[i + 1]) if q != e]
                tally.borderline += int((_band(bmsg[:, others]) & live[:, None]).sum())
                t = np.tanh(bmsg[:, others] / 2.0)
                bad |= (~(np.abs(t) < 1.0)).any(axis=1)
                qv = _ratio(np.prod(t, axis=1))
                near[:, k], border[:, k] = _classify(qv)
                with np.errstate(all="ignore"):
                    cj[:, k] = np.log(qv) * sign[:, i]
            with np.errstate(all="ignore"):
                llr[:, j] = prior[j] + cj.sum(axis=1)
                for k, e in enumerate(own):
                    bmsg[:, e] = prior[j] + np.delete(cj, k, axis=1).sum(axis=1)
            for tile in range(tiles):
                sl = slice(64 * tile, 64 * tile + 64)
                lv = live[sl]
                if not lv.any():
                    continue
                fallback = bool((bad[sl] & lv).any())
                if not fallback:
                    tally.borderline += int((border[sl] & lv[:, None]).sum())
                counts = [int((near[sl, k] & lv).sum()) for k in range(len(own))]
                dead_near = any((near[sl, k] & fresh_dead[sl]).any() and (~near[sl, k] & lv).any() for k in range(len(own)))
                tally.unit(it, tile, j, counts, fallback, dead_near)
        hard = (llr <= 0).astype(np.int64)
        ok = ((hard @ h.T.toarray()) % 2 == s).all(axis=1)
        newly = ok & ~done
        iters[live] = it
        died[newly] = it
        done = done | ok
    return Census(tally.labels, tally.borderline, iters[:batch].copy(), done[:batch] & (died[:batch] > 0), tally.detail)


# ---- codes ----------------------------------------------------------------------------------------------------------------------------------
P_PENDANT = 0.4999  # tanh(prior / 2) = 2e-4: arguments within 1e-3 of 1, where the log's two branches round differently (at 0.49 they mostly agree)
P_SATURATED = 1.0 / (1.0 + np.exp(39.5))  # prior 39.5: tanh is exactly 1 until two checks' messages of about -1.35 each pull it to 36.8
Code = namedtuple("Code", "h probs special")  # special: name -> row / column the syndromes are built around


def _ordinary_priors(rng, n):
    return rng.uniform(0.03, 0.08, size=n)


def _append(h, rows_of_new_columns):
    """h with one new column per entry of the list: the rows that column has entries in."""
    h = sp.lil_matrix(sp.hstack([sp.csr_matrix(h), sp.csr_matrix((h.shape[0], len(rows_of_new_columns)), dtype=np.uint8)]))
    for k, rows in enumerate(rows_of_new_columns):
        for i in rows:
            h[i, h.shape[1] - len(rows_of_new_columns) + k] = 1
    return sp.csr_matrix(h, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def pendant_code(seed, pendants, m=16, n=36, max_row=6, max_col=3, extra=None):
    """A seeded core of m rows (ordinary priors, rows of 2 .. max_row entries) with pendant columns appended: `pendants` = ((row, count), ...),
    rows named by their rank when the core's rows are sorted by weight, heaviest first (rank 0: the row of exactly max_row entries).
    extra = "cancel": a weight-2 row {c, k}, k a pendant with p = 0.30, c (p = 0.29) also in an ordinary row `near_row` -- in a lane whose
        syndrome is that row alone, c tells near_row (0.895 - 0.847) from iteration 2 on, while the lane is dead by then;
    extra = "saturated" / "saturated_w1": a column s with prior 39.5 in two weight-2 rows {s, k2}, {s, k3} (pendants with prior 5): |tanh| = 1 in
        iteration 1 everywhere, and below 1 afterwards where both rows' syndrome bits are set; "_w1" adds a row of ONE entry, on a column of an
        ordinary row, which sends that row +-inf from iteration 2 on."""
    core = lu.build_member(seed, m=m, max_row=max_row, max_col=max_col, min_row=2, n=n)
    rng = np.random.default_rng(seed + 7)
    by_weight = np.argsort(-np.asarray(core.sum(axis=1)).ravel(), kind="stable")
    probs = list(_ordinary_priors(rng, core.shape[1]))
    new, special = [], {}
    for rank, count in pendants:
        new += [[int(by_weight[rank])]] * count
        probs += [P_PENDANT - 0.0002 * k for k in range(count)]
    h = _append(core, new)
    taken = {int(by_weight[rank]) for rank, _ in pendants}
    free = [int(i) for i in by_weight[::-1] if int(i) not in taken]  # lightest first
    if extra == "cancel":
        near_row = free[0]
        h = sp.csr_matrix(sp.vstack([h, sp.csr_matrix((1, h.shape[1]), dtype=np.uint8)]))
        h = _append(h, [[near_row, m], [m]])
        probs += [0.29, 0.30]
        special = dict(near_row=near_row, pair_row=m, rows_to_avoid=(near_row, m))
    elif extra in ("saturated", "saturated_w1"):
        h = sp.csr_matrix(sp.vstack([h, sp.csr_matrix((2, h.shape[1]), dtype=np.uint8)]))
        h = _append(h, [[m, m + 1], [m], [m + 1]])
        probs += [P_SATURATED, 1.0 / (1.0 + np.exp(5.0)), 1.0 / (1.0 + np.exp(4.5))]
        special = dict(sat_rows=(m, m + 1), rows_to_avoid=(m, m + 1))
        if extra == "saturated_w1":
            host = free[0]
            col = int(sp.csr_matrix(h)[host].indices[0])
            row = np.zeros((1, h.shape[1]), np.uint8)
            row[0, col] = 1
            h = sp.csr_matrix(sp.vstack([h, sp.csr_matrix(row)]))
            special.update(w1_row=m + 2, w1_host=host, rows_to_avoid=(m, m + 1, m + 2, host))
    h = sp.csr_matrix(h, dtype=np.uint8)
    h.sort_indices()
    probs = np.array(probs)
    probs.setflags(write=False)
    return Code(h, probs, special)


@functools.lru_cache(maxsize=None)
def regular_code(seed, schedule, saturated=False):
    """A (3,6)-regular 24 x 48 matrix.  Columns 46, 47 (p = 0.4999, 0.4997) share rows 0, 1, 2: their messages stay tiny for ever, so all six
    entries of those rows have near-1 arguments in every lane.  Column 45 (p = 0.49) makes the five other entries of its rows near 1 in
    iteration 1 only.  Column c = 44 is tuned (below) so that, in a lane whose syndrome is column k's, it tells its first row about +0.04
    when that lane has just converged -- live lanes hear a strong message there.  saturated: column 43 gets the prior 41 and strong neighbours: |tanh| = 1 in iteration 1, below 1 afterwards in a lane whose syndrome bits of its three rows are set."""
    rng = np.random.default_rng(seed)
    m, n = 24, 48
    for _ in range(500):
        rest = np.concatenate([np.repeat(np.arange(3, m), 6), np.repeat(np.arange(3), 4)])  # rows 0 .. 2 keep two sockets for columns 46, 47
        rng.shuffle(rest)
        for _ in range(10000):  # a column that repeats a row swaps one of its sockets with a random one
            rows = rest.reshape(n - 2, 3)
            twice = [j for j in range(n - 2) if len(set(rows[j])) < 3]
            if not twice:
                break
            a, b = 3 * twice[0] + int(rng.integers(3)), int(rng.integers(len(rest)))
            rest[a], rest[b] = rest[b], rest[a]
        rows, cols = [list(r) for r in rest.reshape(n - 2, 3)], [[0, 1, 2], [0, 1, 2]]
        if all(len(set(r)) == 3 for r in rows):
            hd = np.zeros((m, n), np.uint8)
            for j, r in enumerate(rows + cols):
                hd[r, j] = 1
            c_rows, w3_rows = set(np.flatnonzero(hd[:, 44])), set(np.flatnonzero(hd[:, 45]))
            sat_rows = set(np.flatnonzero(hd[:, 43]))
            if (hd.sum(axis=1) == 6).all() and not ({0, 1, 2} & (c_rows | w3_rows | sat_rows)) and not (c_rows & w3_rows) and not (sat_rows & (c_rows | w3_rows)):
                break
    else:
        raise AssertionError("no (3,6)-regular matrix with the wanted structure")
    h = sp.csr_matrix(hd)
    probs = _ordinary_priors(rng, n)
    probs[46], probs[47], probs[45] = 0.4999, 0.4997, 0.49
    c = 44
    i, j1, j2 = sorted(c_rows)
    k = next(int(q) for q in np.flatnonzero(hd[j1]) if q not in (c, 43, 45) and not (set(np.flatnonzero(hd[:, q])) & ({i, j2, 0, 1, 2} | sat_rows)))
    probs[k] = 0.40
    if saturated:  # prior 41, between neighbours with p = 1e-4: each of its rows tells it about -+7.6, so it hears 25.8, 41 or 56.2 -- never 38
        probs[np.flatnonzero(hd[sorted(sat_rows)].any(axis=0))] = 1e-4
        probs[43] = 1.0 / (1.0 + np.exp(41.0))
    special = dict(near_row=int(i), k=k, k_rows=tuple(int(r) for r in np.flatnonzero(hd[:, k])), sat_rows=tuple(sorted(int(r) for r in sat_rows)),
                   rows_to_avoid=tuple({0, 1, 2} | c_rows | w3_rows | sat_rows | set(np.flatnonzero(hd[:, k]))))
    # tune c's prior: in the lane with column k's syndrome, the message c -> row i that iteration 2 reads must be about +0.04
    synd = hd[:, k][None, :].astype(np.uint8)
    e_ci = int(h.indptr[i] + np.searchsorted(h.indices[h.indptr[i]:h.indptr[i + 1]], c))
    prior_c = 0.5
    for _ in range(20):  # (the message is the prior plus what the two other rows say, which hardly depends on the prior)
        probs[c] = 1.0 / (1.0 + np.exp(prior_c))
        got = _message_after_first_iteration(h, probs, synd, schedule, e_ci)
        if abs(got - 0.04) < 5e-3:
            break
        prior_c -= got - 0.04
    assert abs(got - 0.04) < 5e-3, got
    probs.setflags(write=False)
    return Code(h, probs, special)


def _message_after_first_iteration(h, probs, synd, schedule, edge):
    """The bit -> check log-ratio of CSR entry `edge` in lane 0 once iteration 1 is over."""
    h, m, n, batch, tiles, s, prior, csc = _setup(h, probs, synd)
    rp = h.indptr
    bmsg = prior[h.indices].copy()
    sign = np.where(s[0] != 0, -1.0, 1.0)
    row_of = np.repeat(np.arange(m), np.diff(rp))

    def check_to_bit(e):
        i = row_of[e]
        t = np.tanh(np.array([bmsg[q] for q in range(rp[i], rp[i + 1]) if q != e]) / 2.0)
        return np.log(_ratio(np.prod(t))) * sign[i]
    if schedule == "parallel":
        c = np.array([check_to_bit(e) for e in range(h.nnz)])
    for j in range(n):
        own = csc.data[csc.indptr[j]:csc.indptr[j + 1]]
        cj = np.array([c[e] if schedule == "parallel" else check_to_bit(e) for e in own])
        for kk, e in enumerate(own):
            bmsg[e] = prior[j] + np.delete(cj, kk).sum()
    return float(bmsg[edge])


# ---- syndromes ------------------------------------------------------------------------------------------------------------------------------
def syndromes(code, seed, tiles_spec, all_set=()):
    """tiles_spec: per tile (lanes, stuck, special) -- `stuck` lanes that never converge (a random error's syndrome at p = 0.04 with one byte set
    to 2, away from the special rows), `special` lanes with the code's special syndrome (the weight-2 row of "cancel" alone / column k's), the
    rest all zero; placed at seeded positions of the tile.  all_set: rows whose syndrome bit is set in every stuck lane."""
    h = code.h
    m, n = h.shape
    rng = np.random.default_rng(seed)
    avoid = set(code.special.get("rows_to_avoid", ()))
    plain = [i for i in range(m) if i not in avoid]
    out = []
    for lanes, stuck, special in tiles_spec:
        s = np.zeros((lanes, m), np.uint8)
        where = rng.permutation(lanes)
        for b in where[:stuck]:
            e = (rng.random(n) < 0.04).astype(np.uint8)
            s[b] = (h @ e) % 2
            s[b, list(avoid)] = 0
            s[b, list(all_set)] = 1
            s[b, int(rng.choice(plain))] = 2
        for b in where[stuck:stuck + special]:
            if "pair_row" in code.special:
                s[b, code.special["pair_row"]] = 1
            else:
                s[b, list(code.special["k_rows"])] = 1
        out.append(s)
    out = np.ascontiguousarray(np.concatenate(out))
    out.setflags(write=False)
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# impl: whose census the case is about (None: a control on the generic routine); shows: labels the census must hold (asserted on the CPU);
# steer: schedule, set_small_code_kernel, set_handoff, set_ring, set_serial_kernel, set_repack, switches -- as tests/stream_ladder_util.py;
# kernel: the instantiation the launch log must show; wave_dr: DR of the bp_wave_ps_kernel rung
NCase = namedtuple("NCase", "id impl code synd max_iter shows steer kernel wave_dr")
Steer = namedtuple("Steer", "schedule mode handoff ring serial_kernel repack switches")
Steer.__new__.__defaults__ = ("parallel", None, None, None, None, None, {})

MAX_ITER = 5
_ROW_SHOWS = ("zero", "under", "at", "over_first", "park_then_over", "dead_near")


def _cases():
    out = []
    # --- check_row, fixed-degree ring form and per-pass form, on the regular code: rows 0 .. 2 hold six near-1 entries per live lane.  Tile 0: 64
    # live lanes in iteration 1 (the first entry alone overflows), 8 from iteration 2 on (8 x 6 = 48: exactly full); tile 1: 9 lanes, all stuck
    # (45 parked, the sixth entry in place; column 45's rows: 9 x 5 = 45 in iteration 1, under)
    reg = lambda: regular_code(21, "parallel")
    reg_synd = lambda: syndromes(reg(), 1, ((64, 8, 12), (9, 9, 0)))
    out.append(NCase("ring-capacity", "check_row", reg, reg_synd, MAX_ITER, _ROW_SHOWS, Steer(mode=0, handoff=0, ring=2), "bp_decode_kernel<0, 0, 6, 3, 2>", None))
    regf = lambda: regular_code(25, "parallel", saturated=True)
    regf_synd = lambda: syndromes(regf(), 2, ((64, 10, 0), (7, 7, 0)), all_set=regf().special["sat_rows"])
    out.append(NCase("ring-fallback", "check_row", regf, regf_synd, MAX_ITER, ("fallback", "fallback_varies", "under", "zero"), Steer(mode=0, handoff=0, ring=2),
                     "bp_decode_kernel<0, 0, 6, 3, 2>", None))
    # --- check_row, variable-degree forms (rows of 2 .. 8 entries under DR = 8): a row of 6 + 2 pendants (8 near-1 entries, row weight = DR), one of
    # 4 + 2 (6 entries), one with one pendant (its other entries), the weight-2 row of "cancel"
    irr = lambda: pendant_code(31, ((0, 2), (6, 2), (10, 1)), extra="cancel")
    irr_synd = lambda: syndromes(irr(), 3, ((64, 8, 12), (9, 9, 0)))
    irr_synd6 = lambda: syndromes(irr(), 4, ((64, 6, 12), (64, 8, 12)))  # 6 live lanes x 8 entries = 48; 128 syndromes
    for name, synd in (("", irr_synd), ("-b128", irr_synd6)):
        out.append(NCase("var-capacity" + name, "check_row", irr, synd, MAX_ITER, _ROW_SHOWS, Steer(mode=0, handoff=0), "bp_decode_kernel<0, 0, 8, 4, 0>", None))
    out.append(NCase("spread-capacity", "check_row", irr, irr_synd, MAX_ITER, _ROW_SHOWS, Steer(mode=0, handoff=1000), "bp_spread_check_kernel<0, 0, 8, 0, false>", None))
    for w1 in (False, True):
        fb = lambda w1=w1: pendant_code(32, ((0, 2), (5, 1)), extra="saturated_w1" if w1 else "saturated")
        fb_synd = lambda fb=fb: syndromes(fb(), 5, ((64, 9, 0), (5, 5, 0)), all_set=fb().special["sat_rows"])
        tag = "-weight1-row" if w1 else ""
        out.append(NCase("var-fallback" + tag, "check_row", fb, fb_synd, MAX_ITER, ("fallback", "fallback_varies", "under", "zero", "park_then_over"), Steer(mode=0, handoff=0),
                         "bp_decode_kernel<0, 0, 8, 4, 0>", None))
        out.append(NCase("spread-fallback" + tag, "check_row", fb, fb_synd, MAX_ITER, ("fallback", "fallback_varies", "under", "zero", "park_then_over"), Steer(mode=0, handoff=1000),
                         "bp_spread_check_kernel<0, 0, 8, 0, false>", None))
    # --- bit_messages: a bit of rows 0 .. 2 of the regular code has up to three near-1 messages per live lane.  16 live lanes x 3 = 48; 17: 34 parked,
    # the third message in place; 64 in iteration 1
    regs = lambda: regular_code(23, "serial")
    regs_synd = lambda: syndromes(regs(), 6, ((64, 16, 12), (17, 17, 0)))
    ser = Steer(schedule="serial", serial_kernel=2, repack=0, switches={"SER_RING": 2})
    out.append(NCase("serial-capacity", "bit_messages", regs, regs_synd, MAX_ITER, _ROW_SHOWS, ser, "bp_serial_stream_kernel<0, 0, 6, 3, 2>", None))
    regsf = lambda: regular_code(26, "serial", saturated=True)
    regsf_synd = lambda: syndromes(regsf(), 7, ((64, 10, 0), (7, 7, 0)), all_set=regsf().special["sat_rows"])
    out.append(NCase("serial-fallback", "bit_messages", regsf, regsf_synd, MAX_ITER, ("fallback", "fallback_varies", "under", "zero"), ser, "bp_serial_stream_kernel<0, 0, 6, 3, 2>", None))
    # the item form of the streamed serial schedule has no parking: the same inputs on the generic routine
    out.append(NCase("serial-var-control", None, irr, irr_synd, MAX_ITER, (), Steer(schedule="serial", serial_kernel=2, repack=0),
                     "bp_serial_stream_var_kernel<0, 0, 8, 4>", None))
    # --- wave: per syndrome and iteration, the near-1 entries of ALL rows against 64 slots.  Pendant pairs on rows of 6 / 5 / 4 ... entries
    wv = Steer(mode=1, switches={"PS_TEAM": 0})
    for name, pend, extra, shows in (("zero", (), None, ("zero",)), ("under", ((0, 2), (1, 2), (2, 1)), None, ("under",)), ("at", "fill:64", None, ("at",)),
                                     ("over", "fill:66", None, ("park_then_over",)), ("fallback", ((0, 2), (1, 2)), "saturated", ("fallback", "fallback_varies", "under")),
                                     ("fallback-weight1-row", ((0, 2), (1, 2)), "saturated_w1", ("fallback",))):
        code = (lambda pend=pend, extra=extra: _wave_code(41, pend, extra))
        synd = (lambda code=code, extra=extra: syndromes(code(), 8, ((64, 20, 0), (6, 6, 0)), all_set=code().special.get("sat_rows", ())))
        dr, dc = (8, 4) if pend else (6, 3)  # pick_wave_ps: the core's rows have 6 entries at most, a row with pendants up to 8
        out.append(NCase("wave-" + name, "wave", code, synd, MAX_ITER, shows, wv, f"bp_wave_ps_kernel<0, {dr}, {dc}, false>", dr))
    # the team form runs the generic routine: same case, same bits
    code = lambda: _wave_code(41, "fill:66", None)
    out.append(NCase("wave-team-control", None, code, lambda: syndromes(code(), 8, ((64, 20, 0), (6, 6, 0))), MAX_ITER, (), Steer(mode=1, switches={"PS_TEAM": 1}),
                     "bp_wave_ps_kernel<0, 8, 4, true>", None))
    return out


def _wave_code(seed, pend, extra):
    """pend "fill:N": pendant pairs on the heaviest rows (each row's every entry near 1) and one pendant on a further row (its other entries)
    so that the near-1 entries of iteration 1 number exactly N."""
    if isinstance(pend, str):
        want = int(pend.split(":")[1])
        core = lu.build_member(seed, m=16, max_row=6, max_col=3, min_row=2, n=36)
        weights = [int(w) for w in np.sort(np.asarray(core.sum(axis=1)).ravel())[::-1]]
        reach = {0: ()}  # near-1 entries -> the pendants that give them, fewest rows first
        for rank, w in enumerate(weights):
            for total, how in sorted(reach.items()):
                for count, adds in ((2, w + 2), (1, w)):
                    if total + adds <= want and total + adds not in reach:
                        reach[total + adds] = how + ((rank, count),)
        assert want in reach, (want, weights)
        pend = reach[want]
        pend = tuple(pend)
    return pendant_code(seed, pend, extra=extra)


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


@functools.lru_cache(maxsize=None)
def census(case_id):
    c = BY_ID[case_id]
    code, synd, cap = c.code(), c.synd(), slot_counts()
    if c.impl == "bit_messages":
        return _with_variation(serial(code.h, code.probs, synd, c.max_iter, cap["bit_messages"]))
    row, wave = flood(code.h, code.probs, synd, c.max_iter, cap["check_row"], c.wave_dr, cap["wave"])
    return _with_variation(wave if c.impl == "wave" else row)


def _with_variation(cs):
    """Adds the label fallback_varies: some row / bit of a tile (some syndrome, for the wave kernel) is left to the generic routine in one
    iteration and takes the parking path in another."""
    seen = {}
    for it, tile, unit, counts, labels in cs.detail:
        seen.setdefault((tile, unit), set()).add("fallback" in labels)
    return cs._replace(labels=cs.labels | ({"fallback_varies"} if any(len(v) == 2 for v in seen.values()) else set()))


@functools.lru_cache(maxsize=None)
def expected(case_id):
    """The oracle's (decoding, llr, iterations, converge) of a case, flooding or serial as the case is."""
    import oracle
    c = BY_ID[case_id]
    code = c.code()
    o = oracle.BpOracle(code.h, error_channel=np.array(code.probs), max_iter=c.max_iter, bp_method="product_sum")
    with np.errstate(all="ignore"):
        return o.decode_serial_batch(c.synd(), None) if c.steer.schedule == "serial" else o.decode_batch(c.synd())
