"""Shared by tests/test_device_math.py (CPU) and tests/test_gpu_device_math.py (GPU): the host build of the device math
(ldpc_amd/csrc/bp_math.h through tests/native/device_math_host.cpp) and the argument sets on which the libm twins are compared -- with the
host libm on the CPU, and with that same host build on the device (ldpc_hip_debug_math_eval)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "device_math_host.cpp")
SO = os.path.join(HERE, "native", "libdevice_math_host.so")
HDR = os.path.join(os.path.dirname(HERE), "ldpc_amd", "csrc", "bp_math.h")
TABLES = os.path.join(os.path.dirname(HERE), "ldpc_amd", "csrc", "bp_libm_tables.h")

_dp = np.ctypeslib.ndpointer(np.float64, flags="C")
_ldp = np.ctypeslib.ndpointer(np.longdouble, flags="C")

# the ranges (lo, hi, drawn in log space) on which tests/test_device_math.py measures the fast routines: tanh_half's |b|, log_pos's q
TANH_HALF_RANGES = ((1e-300, 1e-10, True), (1e-10, 1e-3, True), (1e-3, 2.0, False), (2.0, 10.0, False), (10.0, 37.0, False), (37.0, 39.0, False),
                    (39.0, 1000.0, False))
LOG_POS_RANGES = ((2.0 ** -54, 2.0 ** 54), (0.5, 2.0), (0.99, 1.01), (1 - 1e-8, 1 + 1e-8))


@functools.lru_cache(maxsize=None)
def host_math():
    """libdevice_math_host.so, built when it is older than its sources: g++ -O2 -ffp-contract=off -mfma, as the device build contracts nothing."""
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in (SRC, HDR, TABLES)):
        tmp = f"{SO}.{os.getpid()}.tmp"  # (built aside and moved into place: another test process may be loading or building it)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-o", tmp, SRC], check=True)
        os.replace(tmp, SO)
    lib = C.CDLL(SO)
    for f in ("dm_tanh_half_v", "dm_log_pos_v", "dm_log_ratio_v", "libm_tanh_half_v", "libm_log_v",
              "dx_tanh_half_v", "dx_log_v", "dx_log_ratio_v", "libm_log_ratio_v", "dx_log_split_v", "dx_div_v"):
        getattr(lib, f).argtypes = [C.c_long, _dp, _dp]
    for f in ("ref_tanh_half_v", "ref_log_v"):
        getattr(lib, f).argtypes = [C.c_long, _dp, _ldp]
    for f in ("dm_tanh_half_ptr", "dm_log_ratio_ptr", "dx_tanh_half_ptr", "dx_log_ratio_ptr"):
        getattr(lib, f).restype = C.c_void_p
    return lib


def host_eval(name, arg):
    """One vector routine of the host build on a float64 array (for dx_div_v: [count, 2] pairs) -> a new array of count doubles."""
    arg = np.ascontiguousarray(arg, np.float64)
    count = len(arg)
    out = np.empty(count)
    getattr(host_math(), name)(count, arg.reshape(-1), out)
    return out


def neighbourhood(v, steps=40):
    """v, the `steps` doubles above it and the `steps` doubles below it."""
    e = np.float64(v)
    around = [e]
    for _ in range(steps):
        around.append(np.nextafter(around[-1], np.inf))
    lo_ = e
    for _ in range(steps):
        lo_ = np.nextafter(lo_, -np.inf)
        around.append(lo_)
    return around


# high words of |b| at which the tanh twin's argument reduction or one of its tails changes
TANH_HIGH_WORDS = (0x3fd62e42, 0x3fd62e43, 0x3ff0a2b1, 0x3ff0a2b2, 0x3ff0a2b3, 0x40000000, 0x3fffffff, 0x402a0000, 0x4029ffff, 0x3c900000, 0x3c8fffff,
                   0x40460000, 0x4045ffff)


@functools.lru_cache(maxsize=None)
def twin_arguments():
    """{"b": tanh_half_libm, "q": log_libm, "x": ps_log_ratio_libm, "q_norm": the split log}: about 3 M arguments each (q_norm 2 M), specials, the
    sign of zero and a NaN included; b also holds the neighbourhoods of every threshold of the tanh twin.  Built once; read-only."""
    rng = np.random.default_rng(3)
    n = 1_000_000
    b = np.concatenate([rng.uniform(-100, 100, n), rng.uniform(-4, 4, n),
                        np.exp(rng.uniform(-120, 5, n)) * rng.choice([-1.0, 1.0], n),
                        [0.0, -0.0, np.inf, -np.inf, np.nan, 44.0, 43.99, -44.0, 2e-16, 1e-17, 2.0 ** -54, 2.0 ** -55, 4.0, 2.0, -2.0]])
    q = np.concatenate([np.exp(rng.uniform(-37.5, 37.5, n)), rng.uniform(0.9, 1.1, n), rng.uniform(0.25, 4, n),
                        [0.0, np.inf, np.nan, 1.0, 2.0 ** -54, 2.0 ** 54]])
    x = np.concatenate([rng.uniform(-1, 1, n), np.tanh(rng.uniform(-20, 20, n)), rng.uniform(-1e-3, 1e-3, n),
                        [1.0, -1.0, 0.0, -0.0, np.nan, 1 - 2.0 ** -53, -1 + 2.0 ** -53]])
    # arguments around every threshold of the tanh twin's argument reduction and tails (high-word boundaries, k changes)
    edges = []
    for v in (0.5 * np.log(2) / 1, 1.5 * np.log(2), 2.0, 13.0, 13.5, 20 * np.log(2), 44.0, 2.0 ** -54, 2.0 ** -55, 2.0 ** -1022, 5e-324,
              *(k * np.log(2) for k in range(1, 64)), *((k + 0.5) * np.log(2) for k in range(0, 64))):
        edges.extend(neighbourhood(v))
    hw = np.array(TANH_HIGH_WORDS, dtype=np.uint64)
    words = np.concatenate([(hw << np.uint64(32)) | np.uint64(lo32) for lo32 in (0, 1, 0xffffffff, 0x80000000)]).view(np.float64)
    edges = np.concatenate([np.array(edges, dtype=np.float64), words])
    b = np.concatenate([b, edges, -edges])
    q_norm = np.concatenate([np.exp(rng.uniform(-37.4, 37.4, n)), rng.uniform(0.9, 1.1, n), [1.0, 2.0 ** -54, 2.0 ** 54, 0.9375, np.nextafter(0.9375, 0),
                             1.064697265625, np.nextafter(1.064697265625, 0), np.nextafter(1.0, 0), np.nextafter(1.0, 2)]])
    out = {"b": b, "q": q, "x": x, "q_norm": q_norm}
    for v in out.values():
        v.setflags(write=False)
    return out


# (routine of the host build, the host libm's counterpart, key of twin_arguments): what the CPU test compares bit for bit
TWIN_PAIRS = (("dx_tanh_half_v", "libm_tanh_half_v", "b"), ("dx_log_v", "libm_log_v", "q"), ("dx_log_ratio_v", "libm_log_ratio_v", "x"),
              ("dx_log_split_v", "libm_log_v", "q_norm"))
