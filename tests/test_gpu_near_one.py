"""The near-1 parking of the exact product-sum `log` (check_row_ps_exact_fast, bit_messages_ps_exact_fast, check B of bp_wave_ps_kernel) at and
past its capacity, with dead lanes and with iterations that fall back to the generic routine: every case of tests/near_one_util.py -- whose
census tests/test_near_one_cases.py asserts on the CPU -- decoded with product-sum and the exact math on the kernel family the case names, against
the oracle (flooding: decode_batch; serial: decode_serial_batch): decisions, converge flags and iteration counts equal, log-ratios equal as bit
patterns (oracle.bits_equal), and the launch log shows the family.  A wrong rank, a wrong first slot or the wrong branch for an entry evaluated in
place changes low-order bits of a log-ratio in exactly these cases."""
import numpy as np
import pytest

import launch_util
import near_one_util as nu
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

# every kernel that decodes BP in the families walked here: a case's log shows its own and none of the others
FAMILIES = ("bp_decode_kernel", "bp_spread_check_kernel", "bp_wave_ps_kernel", "bp_wave_kernel", "bp_small_kernel", "bp_edge_kernel", "bp_edge8_kernel",
            "bp_serial_kernel", "bp_serial_level_kernel", "bp_serial_stream_kernel", "bp_serial_stream_var_kernel", "bp_serial_lane_kernel", "bp_serial_lane_var_kernel")


def _decode(case):
    from ldpc_amd.engine import HipBpEngine
    code, synd, st = case.code(), case.synd(), case.steer
    h = code.h
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], np.array(code.probs), case.max_iter, 0, 1.0)
    try:
        if st.schedule != "parallel":
            eng.set_schedule(st.schedule)
        for setter, value in ((eng.set_small_code_kernel, st.mode), (eng.set_handoff, st.handoff), (eng.set_ring, st.ring), (eng.set_serial_kernel, st.serial_kernel),
                              (eng.set_repack, st.repack)):
            if value is not None:
                setter(value)
        for name, value in st.switches.items():
            eng.set_debug_switch(name, value)
        with launch_util.launch_log() as log:
            out = eng.decode_batch(synd)
    finally:
        eng.close()
    return tuple(np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in out), log


@pytest.mark.parametrize("case", nu.CASES, ids=[c.id for c in nu.CASES])
def test_parking_paths_keep_the_oracles_bits(case, oracle_built):
    got, log = _decode(case)
    want = nu.expected(case.id)
    ran = launch_util.of(log, *FAMILIES)
    print(f"{case.id}: launched {ran}")
    launch_util.assert_resolved(log)
    assert ran == [case.kernel], f"expected exactly {case.kernel}; the log has {ran}"
    for k, name in ((0, "decoding"), (2, "iterations"), (3, "converge")):
        assert np.array_equal(got[k], np.asarray(want[k]).astype(got[k].dtype)), name
    if not bits_equal(got[1], want[1]):
        a, b = np.ascontiguousarray(got[1]), np.ascontiguousarray(want[1])
        differ = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
        where = np.argwhere(differ)
        rows = [f"  syndrome {r} bit {j}: kernel {a[r, j]!r} ({a[r, j].hex()}), oracle {b[r, j]!r} ({b[r, j].hex()})" for r, j in where[:8]]
        raise AssertionError(f"log-ratios (bit patterns): {len(where)} of {differ.size} differ, in {len(set(where[:, 0]))} syndromes\n" + "\n".join(rows))
