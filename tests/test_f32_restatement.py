"""The float32 message mode without a GPU: (1) the NumPy restatement the GPU tests compare with (tests/f32_util.py) performs the
reference's operations in the reference's order -- at float64 it equals the C oracle bit for bit on every case of tests/test_gpu_f32.py;
(2) the cases hold what they are chosen for; (3) the ``message_dtype`` property: default, validation, and the combinations float32
refuses, each before any device handle is made."""
import numpy as np
import pytest

import f32_util as fu


def _cases():
    out = [(f"{code}_a{alpha}", lambda code=code, alpha=alpha: fu.small_case(code, alpha))
           for code in ("hamming3", "rep5") for alpha in (0.625, 1.0, 0.0)]
    out += [("degree1_empty", fu.degree1_case), ("irregular600", fu.irregular_case), ("bb144", fu.bb144_case), ("heavy_rows", fu.heavy_rows_case)]
    return out


@pytest.mark.parametrize("key,make", _cases(), ids=[k for k, _ in _cases()])
def test_float64_restatement_equals_the_oracle(oracle_built, key, make):
    c = make()
    want = oracle_built.BpOracle(c["h"], error_channel=c["probs"], max_iter=c["max_iter"], bp_method="minimum_sum",
                                 ms_scaling_factor=c["alpha"]).decode_batch(c["synd"])
    dec, llr, it, cv = fu.expected(key, c, np.float64)
    assert np.array_equal(dec, want[0]), "hard decisions"
    assert np.array_equal(cv, want[3]), "converge flags"
    assert np.array_equal(it, want[2]), "iteration counts"
    assert oracle_built.bits_equal(llr, want[1]), "log-ratios differ in some bit"


def test_float32_values_are_float32_and_differ_from_float64():
    c = fu.irregular_case()
    llr32 = fu.expected("irregular600", c, np.float32)[1]
    llr64 = fu.expected("irregular600", c, np.float64)[1]
    assert np.array_equal(llr32, llr32.astype(np.float32).astype(np.float64)), "every float32-mode log-ratio is a widened float32"
    assert not np.array_equal(llr32, llr64), "the two modes must differ somewhere, or the GPU comparison proves nothing"


def test_irregular_case_has_early_stops_and_failures():
    c = fu.irregular_case()
    _, _, it, cv = fu.expected("irregular600", c, np.float32)
    print(f"irregular600 float32: {int(cv.sum())} of {len(cv)} rows converge, iterations {np.bincount(it)}")
    assert (cv & (it < c["max_iter"])).any(), "no row stops early"
    assert (~cv).any(), "every row converges"
    assert len(set(it[cv])) > 2, "the rows that converge all stop at the same iteration"


def test_bb144_case_leaves_rows_for_osd():
    c = fu.bb144_case()
    cv = fu.expected("bb144", c, np.float32)[3]
    print(f"bb144 float32: {int((~cv).sum())} of {len(cv)} rows unconverged")
    assert int((~cv).sum()) >= 10


def test_edge_syndromes_are_what_the_issue_asks():
    s = fu.small_case("hamming3", 0.625)["synd"]
    assert s.shape[0] == 70 and not s[5].any() and (s[9] == 2).any() and (s[66] == 3).any()
    for a in (0.625, 1.0, 0.0):
        cv = fu.expected(f"hamming3_a{a}", fu.small_case("hamming3", a), np.float32)[3]
        assert not cv[9] and not cv[66], "a syndrome byte > 1 never converges"


def _simulated_lists(end):
    """The device's tile list before each compaction (host_f32.h: rounds 4, 8, 12; bp_f32_compact_kernel keeps a tile whose last round,
    0-based ``end - 1``, is not before the compaction's) -> [(round, list)], and the list after the last one."""
    lst, out = list(range(len(end))), []
    for r in fu.COMPACTION_ROUNDS:
        out.append((r, lst))
        lst = [t for t in lst if r <= end[t] - 1]
    return out, lst


def test_standard_schedule_has_the_properties_the_gpu_tests_rely_on():
    """Derived from the restatement's outputs alone: per-tile end iteration = the largest of its rows, and the list each compaction sees."""
    case, idx, synd, want = fu.standard_schedule()
    base = fu.expected("irregular600", case, np.float32)
    max_iter = case["max_iter"]
    assert max_iter == 16 and len(idx) == 69 * 64 + 7 == 4423 and synd.shape == (4423, 300)
    assert all(np.array_equal(w, x[idx]) for w, x in zip(want, base)) and np.array_equal(synd, case["synd"][idx])
    end = fu.tile_end_iterations(base, idx, max_iter)
    print(f"standard schedule: tile end iterations {end.tolist()}")
    assert len(end) == 70 and end.tolist() == list(fu.STANDARD_FINISH), "a tile does not end at the iteration the schedule gives it"
    row_end = fu.row_end_iterations(want, max_iter)
    for t in np.flatnonzero(end == max_iter):
        assert not want[3][64 * t:64 * t + 64].all(), f"tile {t} runs to the end without an unconverged row"
    for lo, hi in ((1, 4), (5, 8), (9, 12), (13, 16)):
        assert ((row_end >= lo) & (row_end <= hi)).any(), f"no row ends in iterations {lo} .. {hi}"
    steps = np.diff(end)
    assert (steps > 0).any() and (steps < 0).any() and sorted(end) != end.tolist(), "end iterations in order"
    lists, left = _simulated_lists(end)
    for r, lst in lists:
        ended = [end[t] - 1 < r for t in lst]
        print(f"compaction at round {r}: {len(lst)} tiles listed, {sum(ended)} of them final ({sum(ended[64:])} beyond slot 63)")
        assert len(lst) > 64, f"round {r}: the list has no second chunk of 64"
        assert any(ended[:64]), f"round {r}: no final tile among the first 64 slots (nothing moves: kept == s0)"
        assert not all(ended[64:]), f"round {r}: no running tile beyond slot 63 (kept is never carried into the second chunk)"
        # a tile that became final before the round just before this compaction stayed listed: the kernels had to skip it
        assert any(end[t] - 1 < r - 1 for t in lst), f"round {r}: no tile ended between two compactions"
    assert left and all(end[t] == max_iter for t in left) and len(left) == int((end == max_iter).sum())
    full = np.flatnonzero(end == max_iter)
    assert (full < 64).any() and (full >= 64).any(), "tiles that run to the end in one chunk only"
    assert end[-1] == max_iter and len(idx) % 64 == fu.STANDARD_LAST_ROWS, "the partial tile must run to the end"
    for t in range(69):
        rows = min(64, len(idx) - 64 * (t + 1))
        assert not np.array_equal(idx[64 * t:64 * t + rows], idx[64 * (t + 1):64 * (t + 1) + rows]), f"tiles {t} and {t + 1} hold the same rows"
        assert not np.array_equal(synd[64 * t:64 * t + rows], synd[64 * (t + 1):64 * (t + 1) + rows])
    again = fu.scheduled_batch(case, base, fu.STANDARD_FINISH, fu.STANDARD_LAST_ROWS, 2024)
    assert np.array_equal(again[0], idx), "the builder is not deterministic in its seed"


def test_converging_schedule_and_its_restatement_at_a_huge_max_iter():
    """What the early-stop GPU test decodes: every row converges, the slowest at iteration 12, and 200 000 allowed iterations give those
    rows exactly what 16 give them."""
    case, idx, synd, want = fu.standard_schedule(converging_only=True)
    base = fu.expected("irregular600", case, np.float32)
    assert want[3].all() and int(want[2].max()) == 12 and len(idx) == 4423
    end = fu.tile_end_iterations(base, idx, case["max_iter"])
    assert end.tolist() == [min(f, 12) for f in fu.STANDARD_FINISH]
    rows, huge = fu.converging_rows_expected(200000)
    assert set(idx.tolist()) <= set(rows.tolist())
    assert int(huge[2].max()) == 12 and huge[3].all()
    for got, x in zip(huge, base):
        assert np.array_equal(got.view(np.uint64) if got.dtype == np.float64 else got, x[rows].view(np.uint64) if x.dtype == np.float64 else x[rows])


def test_edge_value_batches_mix_tiles_that_end_at_once_with_tiles_that_never_do():
    for code, alpha in (("hamming3", 0.625), ("rep5", 0.0)):
        case, idx, synd, want = fu.edge_values_batch(code, alpha)
        base = fu.expected(f"{code}_a{alpha}", case, np.float32)
        end = fu.tile_end_iterations(base, idx, case["max_iter"])
        assert len(end) == 70 and len(idx) == 69 * 64 + 6
        quick = np.arange(70) % 3 == 1
        assert (end[quick] <= 2).all() and (end[~quick] == case["max_iter"]).all(), end.tolist()
        assert (synd == 2).any() and (synd == 3).any() and (~synd.any(axis=1)).any() and np.isinf(want[1]).any()
        lists, _ = _simulated_lists(np.where(end < 4, end, 16))  # (12 iterations: compactions at rounds 4 and 8; nothing ends in between)
        r, lst = lists[0]
        assert r == 4 and any(end[t] <= 2 for t in lst[:64]) and any(end[t] > 2 for t in lst[64:])
        for t in range(69):
            rows = min(64, len(idx) - 64 * (t + 1))
            assert not np.array_equal(idx[64 * t:64 * t + rows], idx[64 * (t + 1):64 * (t + 1) + rows]), f"{code}: tiles {t} and {t + 1} hold the same rows"
        invalid = [bool((synd[64 * t:64 * t + 64] > 1).any()) for t in range(70)]
        assert not any(np.array(invalid)[quick]) and sum(invalid) >= 20 and any(invalid[64:]), "tiles with a syndrome byte > 1: too few, or none in the second chunk"


# ---- the property -----------------------------------------------------------------------------------------------------------------
def _decoder(cls=None, **kw):
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.codes import hamming_code
    kw.setdefault("error_rate", 0.1)
    kw.setdefault("bp_method", "minimum_sum")
    return (cls or BpDecoder)(hamming_code(3), **kw)


def test_message_dtype_default_and_setter():
    d = _decoder()
    assert d.message_dtype == "float64"
    for value, want in (("float32", "float32"), ("float64", "float64"), (np.float32, "float32"), (np.float64, "float64")):
        d.message_dtype = value
        assert d.message_dtype == want
    for bad in ("float16", "f32", np.float16, 32, None, float, np.dtype("float32").itemsize):
        with pytest.raises(ValueError, match="message_dtype"):
            d.message_dtype = bad
    assert d.message_dtype == "float64", "a refused value leaves the property as it was"


def test_message_dtype_is_not_a_constructor_keyword():
    with pytest.raises(ValueError, match="Unknown parameter"):
        _decoder(message_dtype="float32")


SYND = np.array([1, 0, 1], np.uint8)


def test_float32_refuses_product_sum():
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    d = _decoder(bp_method="product_sum")
    d.message_dtype = "float32"
    with pytest.raises(NotImplementedError, match="product_sum"):
        d.decode(SYND)
    with pytest.raises(NotImplementedError, match="product_sum"):
        d.decode_batch(SYND[None, :])
    o = _decoder(BpOsdDecoder, bp_method="product_sum", osd_method="osd_0")
    o.message_dtype = np.float32
    with pytest.raises(NotImplementedError, match="product_sum"):
        o.decode(SYND)
    with pytest.raises(NotImplementedError, match="product_sum"):
        o.decode_batch(SYND[None, :])
    assert d._engine is None and o._engine is None, "refused before any device handle is made"


@pytest.mark.parametrize("schedule", ["serial", "serial_relative"])
def test_float32_refuses_serial_schedules(schedule):
    d = _decoder(schedule=schedule)
    d.message_dtype = "float32"
    with pytest.raises(NotImplementedError, match="schedule"):
        d.decode(SYND)
    with pytest.raises(NotImplementedError, match="schedule"):
        d.decode_batch(SYND[None, :])
    assert d._engine is None


def test_float32_refuses_row_priors_device_ids_and_soft_info():
    from ldpc_amd.bp_decoder import SoftInfoBpDecoder
    d = _decoder()
    d.message_dtype = "float32"
    with pytest.raises(NotImplementedError, match="channel_probs"):
        d.decode_batch(SYND[None, :], channel_probs=np.full((1, 7), 0.1))
    m = _decoder(device_ids=[0, 1])
    m.message_dtype = "float32"
    with pytest.raises(NotImplementedError, match="device_ids"):
        m.decode_batch(SYND[None, :])
    s = _decoder(SoftInfoBpDecoder)
    s.message_dtype = "float32"
    with pytest.raises(NotImplementedError, match="soft-syndrome"):
        s.decode(np.array([0.5, -0.5, 1.0]))
    assert d._engine is None and m._engine is None and s._engine is None


def test_all_zero_shortcut_needs_no_device_in_float32():
    d = _decoder()
    d.message_dtype = "float32"
    assert not d.decode(np.zeros(3, np.uint8)).any() and d.converge
