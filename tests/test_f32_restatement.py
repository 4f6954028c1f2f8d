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
