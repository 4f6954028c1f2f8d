"""The DEVICE compile of ldpc_amd/csrc/bp_math.h, evaluated argument by argument (ldpc_hip_debug_math_eval) and compared bit for bit with the
HOST compile of the same header (tests/native/device_math_host.cpp), which tests/test_device_math.py pins to the host libm on the CPU.

The two compiles differ where it matters: div_cr is a reciprocal + FMA sequence on the device and `/` on the host, fma_kk is inline assembly on
the device, and LDPC_ANY is a wavefront ballot on the device -- if any lane of a wavefront holds a rare argument, every lane runs the rare block.
(1) bit equality on the shared argument sets (tests/device_math_util.py), on division operands of div_cr's three call sites and on the fast
    routines' ranges;
(2) neighbour independence: a lane's result does not depend on what the other 63 lanes of its wavefront hold -- wavefronts of common arguments,
    of common arguments around ONE rare one (lane 0, 31, 63; every rare kind), and of rare arguments only; every element equals the host's, and
    eval(x[perm]) == eval(x)[perm].
Every comparison is on raw bit patterns: the payload of a NaN and the sign of a zero count."""
import numpy as np
import pytest

import device_math_util as dmu

pytestmark = pytest.mark.gpu

# which -> (name in ldpc_amd.engine.MATH_ROUTINES, routine of the host build)
ROUTINES = {0: ("tanh_half_libm", "dx_tanh_half_v"), 1: ("log_libm", "dx_log_v"), 2: ("ps_log_ratio_libm", "dx_log_ratio_v"),
            3: ("log_split", "dx_log_split_v"), 4: ("div_cr", "dx_div_v"), 5: ("tanh_half", "dm_tanh_half_v"), 6: ("ps_log_ratio", "dm_log_ratio_v")}
LN2 = float(np.log(2.0))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _device(which, arg):
    import torch
    from ldpc_amd import engine
    assert engine.MATH_ROUTINES[which] == ROUTINES[which][0]
    out = engine.debug_math_eval(which, torch.tensor(np.asarray(arg, np.float64), device="cuda"))
    return out.cpu().numpy()


def _assert_same_bits(which, arg, got, want, what):
    differ = np.flatnonzero(_bits(got) != _bits(want))
    if len(differ):
        rows = [f"  {ROUTINES[which][0]}({', '.join(float(v).hex() for v in np.atleast_1d(arg[i]))}) [element {i}, lane {i % 64}]: "
                f"device {_bits(got)[i]:#018x} ({got[i]!r}), host {_bits(want)[i]:#018x} ({want[i]!r})" for i in differ[:12]]
        raise AssertionError(f"{what}: {len(differ)} of {len(got)} results differ from the host build\n" + "\n".join(rows))


def _div_pairs():
    """(numerator, denominator) pairs of div_cr's three call sites, with the 40 doubles on either side of each range end."""
    rng = np.random.default_rng(11)
    n = 300_000
    near = lambda v: np.array(dmu.neighbourhood(v))
    sign = lambda k: rng.choice([-1.0, 1.0], k)
    # 1. expm1's rational term: r1 - tt is about -2 (and can be any small number), 6 - x tt lies in [5.6, 6.4]
    den1 = np.concatenate([rng.uniform(5.6, 6.4, 2 * n), near(5.6), near(6.4), near(6.0)])
    num1 = np.concatenate([rng.uniform(-2.6, -1.4, n), np.exp(rng.uniform(-40, 1, n)) * sign(n), np.full(3 * 81, -2.0)])
    # 2. tanh from expm1: 2 / (t + 2) for |x| >= 1, -t / (t + 2) for |x| < 1; t + 2 in [1.1, 2^64]
    den2 = np.concatenate([np.exp(rng.uniform(np.log(1.1), 64 * LN2, n)), rng.uniform(1.1, 2.0, n), near(1.1), near(2.0), near(2.0 ** 64)])
    small = den2[den2 < 2.0]  # (t = 0 belongs to the tiny patch, not to this division)
    num2 = np.concatenate([np.full(len(den2), 2.0), -(small - 2.0)])
    den2 = np.concatenate([den2, small])
    # 3. the message's ratio (1 + x) / (1 - x), |x| < 1, down to 1 - x = 2^-53
    below_one = near(np.nextafter(1.0, 0.0))
    below_one = below_one[below_one < 1.0]
    x = np.concatenate([rng.uniform(-1, 1, n), np.tanh(rng.uniform(-20, 20, n)), rng.uniform(-1e-3, 1e-3, n), 1.0 - 2.0 ** -np.arange(1.0, 54.0),
                        -(1.0 - 2.0 ** -np.arange(1.0, 54.0)), below_one, -below_one, near(0.0), [0.0, -0.0]])
    x = x[np.abs(x) < 1.0]  # (tanh saturates to exactly 1 from 19.1 on: the caller handles that)
    assert (1.0 - x).min() == 2.0 ** -53 and (1.0 + x).min() == 2.0 ** -53
    pairs = np.stack([np.concatenate([num1, num2, 1.0 + x]), np.concatenate([den1, den2, 1.0 - x])], axis=1)
    return np.ascontiguousarray(pairs)


def _fast_tanh_arguments():
    rng = np.random.default_rng(5)
    out = []
    for lo, hi, logspace in dmu.TANH_HALF_RANGES:
        b = np.exp(rng.uniform(np.log(lo), np.log(hi), 200_000)) if logspace else rng.uniform(lo, hi, 200_000)
        out.append(b * rng.choice([-1.0, 1.0], len(b)))
    return np.concatenate(out + [[0.0, -0.0, np.inf, -np.inf, np.nan, 38.0, 38.2, -50.0, 1e308]])


def _fast_log_ratio_arguments():
    """x with (1 + x) / (1 - x) spread over log_pos's ranges, and the ends of ps_log_ratio's domain."""
    rng = np.random.default_rng(6)
    q = np.concatenate([np.exp(rng.uniform(np.log(lo), np.log(hi), 200_000)) for lo, hi in dmu.LOG_POS_RANGES])
    x = (q - 1.0) / (q + 1.0)
    return np.concatenate([x, [1.0, -1.0, 0.0, -0.0, np.nan, np.nextafter(1.0, 0.0), -np.nextafter(1.0, 0.0)]])


def _arguments(which):
    shared = dmu.twin_arguments()
    if which <= 3:
        return shared[("b", "q", "x", "q_norm")[which]]
    return (_div_pairs, _fast_tanh_arguments, _fast_log_ratio_arguments)[which - 4]()


@pytest.mark.parametrize("which", sorted(ROUTINES), ids=[ROUTINES[w][0] for w in sorted(ROUTINES)])
def test_device_build_equals_the_host_build_bit_for_bit(which):
    arg = _arguments(which)
    want = dmu.host_eval(ROUTINES[which][1], arg)
    got = _device(which, arg)
    print(f"{ROUTINES[which][0]}: {len(want)} arguments")
    _assert_same_bits(which, arg, got, want, "device build vs host build")


# ---- neighbour independence ----------------------------------------------------------------------------------------------------------------
def _tanh_k(b):
    """The k of the twin's argument reduction (bp_math.h: tanh_half_libm) for a common |b|."""
    a = abs(float(b))
    if a < 2.0:
        return int(-a / LN2 - 0.5) if a > 0.5 * LN2 else 0
    return int(a / LN2 + 0.5)


def _tanh_common():
    """|b| in [2^-54, 13): no lane rare.  Both signs, every k the tails select on: -3 .. 0 below |b| = 2, 3 .. 19 from there on (k = 1 never
    occurs, and k = 2 needs |b| < 1.74 on the side where |b| >= 2)."""
    mags = [1e-12, 1e-3, 0.1, 0.3, 0.346, 0.35, 0.6, 0.9, 1.0, 1.03, 1.05, 1.3, 1.6, 1.73, 1.74, 1.9, np.nextafter(2.0, 0.0), 2.0, 2.05, 2.3, 2.5]
    mags += [(k + u) * LN2 for k in range(4, 19) for u in (-0.45, 0.0, 0.45)] + [18.6 * LN2, 18.7 * LN2, np.nextafter(13.0, 0.0)]
    mags = np.array(mags)
    assert mags.min() >= 2.0 ** -54 and mags.max() < 13.0
    ks = {_tanh_k(v) for v in mags}
    assert ks == {-3, -2, -1, 0} | set(range(3, 20)), sorted(ks)
    return np.concatenate([mags, -mags])


def _tanh_random(rng, k):
    """Common arguments drawn at random: |b| uniform in [0, 13) or log-uniform down to 2^-54, either sign."""
    mags = np.where(rng.random(k) < 0.8, rng.uniform(0.0, 13.0, k), np.exp(rng.uniform(np.log(2.0 ** -54), np.log(2.0), k)))
    return np.clip(mags, 2.0 ** -54, np.nextafter(13.0, 0.0)) * rng.choice([-1.0, 1.0], k)


NEIGHBOUR = {
    # which: (the common arguments every case holds, common arguments drawn at random, {rare kind: arguments})
    0: (_tanh_common, _tanh_random, {
        "rare, k < 20": [13.0, 13.2, -13.4, 13.51],
        "k >= 20": [13.52, -13.9, 14.0, 20.0, -30.0, 43.9],
        "|b| >= 44": [44.0, -50.0, 1e308],
        "infinite": [np.inf, -np.inf],
        "NaN": [np.nan, -np.nan],
        "zero": [0.0, -0.0],
        "subnormal": [5e-324, -1e-310],
        "|b| < 2^-54": [1e-17, -(2.0 ** -55), np.nextafter(2.0 ** -54, 0.0)],
    }),
    1: (lambda: np.array([1.0, 0.9375, np.nextafter(0.9375, 0.0), 1.064697265625, np.nextafter(1.064697265625, 0.0), 2.0 ** -54, 2.0 ** 54, 0.5, 2.0]),
        lambda rng, k: np.where(rng.random(k) < 0.6, np.exp(rng.uniform(-37, 37, k)), rng.uniform(0.93, 1.07, k)),
        {"zero": [0.0], "+inf": [np.inf], "NaN": [np.nan]}),
    2: (lambda: np.array([0.0, -0.0, 0.03, -0.03, 0.5, -0.5, np.nextafter(1.0, 0.0), -np.nextafter(1.0, 0.0)]),
        lambda rng, k: np.where(rng.random(k) < 0.6, rng.uniform(-1.0, 1.0, k), np.tanh(rng.uniform(-18, 18, k))),
        {"x = 1": [1.0], "x = -1": [-1.0], "NaN": [np.nan]}),
}
RANDOM_WAVEFRONTS = 400  # x 63 common lanes beside one rare lane: a tail that leaks into a common lane changes about 5 results in 1000 there


def _wavefronts(which):
    """-> (arguments, a label per wavefront): (a) all common, (b) 63 common lanes and one rare lane -- at lane 0, 31, 63 for every rare value, then
    at a random lane among common arguments drawn at random --, (c) all rare."""
    pool_fn, random_fn, rare = NEIGHBOUR[which]
    rng = np.random.default_rng(30 + which)
    pool = pool_fn()
    common = np.concatenate([pool, random_fn(rng, 64 * 6 - len(pool) % 64)])
    every = np.array([v for values in rare.values() for v in values])
    waves, labels = [], []
    order = rng.permutation(len(common))
    for s in range(0, len(common) - 63, 64):  # (a): every pooled common argument at least once
        waves.append(common[order[s:s + 64]])
        labels.append("all common")
    for kind, values in rare.items():  # (b)
        for v in values:
            for lane in (0, 31, 63):
                w = np.concatenate([rng.choice(pool, 32), random_fn(rng, 32)])
                w[lane] = v
                waves.append(w)
                labels.append(f"one rare lane ({kind}: {v!r}) at lane {lane}")
    for _ in range(RANDOM_WAVEFRONTS):
        w = random_fn(rng, 64)
        lane, v = int(rng.integers(64)), rng.choice(every)
        w[lane] = v
        waves.append(w)
        labels.append(f"random common lanes around one rare lane ({v!r}) at lane {lane}")
    for _ in range(3):  # (c)
        waves.append(rng.choice(every, 64))
        labels.append("all rare")
    return np.concatenate(waves), labels


@pytest.mark.parametrize("which", sorted(NEIGHBOUR), ids=[ROUTINES[w][0] for w in sorted(NEIGHBOUR)])
def test_a_lane_keeps_its_bits_whatever_its_neighbours_hold(which):
    arg, labels = _wavefronts(which)
    assert len(arg) == 64 * len(labels)
    want = dmu.host_eval(ROUTINES[which][1], arg)
    got = _device(which, arg)
    differ = np.flatnonzero(_bits(got) != _bits(want))
    if len(differ):
        bad = sorted({labels[i // 64] for i in differ})
        _assert_same_bits(which, arg, got, want, "wavefronts " + "; ".join(bad[:6]))
    perm = np.random.default_rng(40 + which).permutation(len(arg))  # (lanes change wavefronts: rare lanes meet other neighbours)
    moved = _device(which, arg[perm])
    _assert_same_bits(which, arg[perm], moved, got[perm], "eval(x[perm]) vs eval(x)[perm]")
