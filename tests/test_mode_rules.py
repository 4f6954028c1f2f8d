"""What each decode mode refuses (float32 messages, memory min-sum, Relay-BP, guided decimation), text for text, without a GPU.

Two walks over every combination of settings, each compared with a file under tests/golden/ that was recorded on the commit BEFORE the rules
became one table (ldpc_amd/csrc/mode_host.h, ``BpDecoderBase._require_modes``) -- from the four hand-written ladders of that commit, never
from the table: the C rules through tools/mode_host_check.cpp (built with the host sanitizers, run on its own), the Python rules through the
decoders' public calls.  Both files hold the distinct answers once and one index per state, in the order of the walk."""
import itertools
import json
import os
import shutil
import subprocess

import numpy as np

import f32_util as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _compare(name, states):
    """``states``: (description, answer) pairs in the order of the walk."""
    want = json.load(open(os.path.join(GOLDEN, name)))
    assert len(states) == len(want["states"]), f"{name}: the walk has {len(states)} states, the file {len(want['states'])}"
    refused = 0
    for (state, got), k in zip(states, want["states"]):
        assert got == want["answers"][k], f"{name}: {state}\n  now:    {got}\n  before: {want['answers'][k]}"
        refused += got not in ("0", "accepted")
    assert refused > len(states) // 2 and refused < len(states), "the walk shows refusals and acceptances"


# ---- C: mode_refusal / mode_exclusion of mode_host.h ----------------------------------------------------------------------------------------
def test_c_rules_answer_as_the_four_ladders_did(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (build() uses one too)"
    exe = str(tmp_path / "mode_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "ldpc_amd", "csrc"), os.path.join(ROOT, "tools", "mode_host_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr
    lines = run.stdout.splitlines()
    assert lines[-1] == "mode_host_check ok"
    _compare("mode_rules_c.json", [(f"line {i + 1} of mode_host_check's output", line) for i, line in enumerate(lines[:-1])])


# ---- Python: the decoders' calls, each stopped where it would make a handle -------------------------------------------------------------------
class _Accepted(Exception):
    pass


def _stop(*args, **kw):
    raise _Accepted


def _answer(call):
    try:
        out = call()
    except _Accepted:
        return "accepted"
    except Exception as exc:  # noqa: BLE001 (the type is part of the answer)
        return f"{type(exc).__name__}: {exc}"
    return f"returned {out!r}"


def python_states():
    from ldpc_amd.bp_decoder import BpDecoder, SoftInfoBpDecoder
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    from ldpc_amd.codes import hamming_code
    codes = (("hamming3", hamming_code(3)), ("irregular600", fu.irregular_case(batch=1)["h"]))  # bp_edge8 takes the first, no ladder the second
    states = []
    for (code, h), f32, mem, relay, gd, method, schedule, random_serial, device_ids, p0 in itertools.product(
            codes, (False, True), (False, True), (False, True), (False, True), ("product_sum", "minimum_sum"),
            ("parallel", "serial", "serial_relative"), (False, True), (None, [0]), (False, True)):
        m, n = h.shape
        channel = [0.0 if p0 and j == 0 else 0.05 for j in range(n)]
        kw = dict(error_channel=channel, max_iter=5, bp_method=method, ms_scaling_factor=0.625, schedule=schedule, device_ids=device_ids)
        synd, soft, probs = np.ones((2, m), np.uint8), np.ones((2, m)), np.full((2, n), 0.05)

        def made(cls, **more):
            d = cls(h, **dict(kw, **more))
            d._get_engine = d._get_cy = _stop
            d.random_serial_schedule = random_serial
            if f32:
                d.message_dtype = "float32"
            if mem:
                d.memory_strength = 0.3
            if relay:
                d.relay = dict(num_sets=2, pre_iter=4, set_max_iter=3)
            if gd:
                d.decimation = dict(round_iters=3, max_rounds=4)
            return d
        tag = (f"{code} float32={f32} memory={mem} relay={relay} decimation={gd} {method} {schedule} random_serial={random_serial} "
               f"device_ids={device_ids} p[0]={channel[0]}")
        calls = [("BpDecoder.decode_batch", lambda: made(BpDecoder, input_vector_type="syndrome").decode_batch(synd)),
                 ("BpDecoder.decode_batch(channel_probs=)", lambda: made(BpDecoder, input_vector_type="syndrome").decode_batch(synd, channel_probs=probs)),
                 ("BpDecoder.decode", lambda: made(BpDecoder, input_vector_type="syndrome").decode(synd[0])),
                 ("BpDecoder.relay_route", lambda: made(BpDecoder).relay_route),
                 ("BpDecoder.decimation_route", lambda: made(BpDecoder).decimation_route),
                 ("SoftInfoBpDecoder.decode", lambda: made(SoftInfoBpDecoder).decode(soft[0])),
                 ("SoftInfoBpDecoder.decode_batch", lambda: made(SoftInfoBpDecoder).decode_batch(soft))]
        for osd, order in (("osd_0", 0), ("osd_e", 2), ("osd_cs", 2)):
            calls += [(f"BpOsdDecoder({osd}).decode_batch", lambda osd=osd, order=order: made(BpOsdDecoder, osd_method=osd, osd_order=order).decode_batch(synd)),
                      (f"BpOsdDecoder({osd}).decode_batch(channel_probs=)",
                       lambda osd=osd, order=order: made(BpOsdDecoder, osd_method=osd, osd_order=order).decode_batch(synd, channel_probs=probs)),
                      (f"BpOsdDecoder({osd}).decode", lambda osd=osd, order=order: made(BpOsdDecoder, osd_method=osd, osd_order=order).decode(synd[0]))]
        states += [(f"{tag}: {name}", _answer(call)) for name, call in calls]
    return states


def test_python_rules_answer_as_the_four_methods_did():
    _compare("mode_rules_python.json", python_states())
