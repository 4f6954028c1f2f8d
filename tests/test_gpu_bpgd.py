"""BP with guided decimation on the device (ldpc_hip_bp_set_decimation) against the NumPy restatement
(tests/bpgd_util.py), bit for bit: hard decisions, converge flags, total iteration counts and the bit patterns of the posteriors -- on the
lane = edge decimation kernels (bp_edge_gd_kernel, bp_edge8_gd_kernel: every instantiation once), with the launch log showing which kernel
ran; rows pulled from the work pools into poisoned outputs; then what goes round them: one round against the plain decode, off / on /
off, new channel probabilities, the adaptive alpha, ties, nothing left to freeze, infinite priors and an infinite freeze value, the decoder classes, BP + OSD-0, the detector-error-model loop, the
refusals of the C ABI, and that close() frees every buffer.

Every comparison first asserts ON THE RESTATEMENT'S OUTPUT what the batch shows: a row solved in round 0, a row solved after at least one
decimation, a row that walks every round (bpgd_util.shows)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import bpgd_util as gu
import f32_util as fu
import ladder_util as lu
import launch_util
import mem_bp_util as mu
from oracle import bits_equal

pytestmark = pytest.mark.gpu

EDGE_GD = ("bp_edge_gd_kernel", "bp_edge8_gd_kernel")
OTHER_VARIANTS = ("bp_edge_rp_kernel", "bp_edge8_rp_kernel", "bp_edge_f32_kernel", "bp_edge8_f32_kernel", "bp_edge_mem_kernel", "bp_edge8_mem_kernel",
                  "bp_edge_relay_kernel", "bp_edge8_relay_kernel", "bp_wave_relay_kernel", "relay_select_kernel")
PLAIN_BP = tuple(lu.BP_DECODE_KERNELS) + OTHER_VARIANTS


def _same(got, want, what):
    dec, llr, it, cv = got[:4]
    print(f"{what}: {int(np.count_nonzero(np.asarray(dec) != want[0]))} decisions, {int(np.count_nonzero(np.asarray(cv, bool) != want[3]))} flags, "
          f"{int(np.count_nonzero(np.asarray(it) != want[2]))} iteration counts differ, "
          f"{int(np.count_nonzero(np.ascontiguousarray(llr, np.float64).view(np.uint64) != np.ascontiguousarray(want[1]).view(np.uint64)))} posteriors differ in some bit")
    odd = np.flatnonzero((np.asarray(it) != want[2]) | (np.asarray(cv, bool) != want[3]))[:8]
    if len(odd):
        print(f"{what}: rows {odd.tolist()}: iterations {np.asarray(it)[odd].tolist()} for {want[2][odd].tolist()}, "
              f"flags {np.asarray(cv, bool)[odd].astype(int).tolist()} for {want[3][odd].astype(int).tolist()}")
    assert np.array_equal(np.asarray(dec), want[0]), f"{what}: hard decisions"
    assert np.array_equal(np.asarray(cv, bool), want[3]), f"{what}: converge flags"
    assert np.array_equal(np.asarray(it), want[2]), f"{what}: iteration counts"
    assert bits_equal(np.asarray(llr), want[1]), f"{what}: posteriors differ in some bit"


def _engine(c, gd=True, mode=None, max_iter=12, switches=None):
    from ldpc_amd.engine import HipBpEngine
    h = sp.csr_matrix(c["h"])
    eng = HipBpEngine(h.indptr, h.indices, h.shape[1], c["probs"], c.get("max_iter", max_iter), 1, c["alpha"])
    if mode is not None:
        eng.set_small_code_kernel(mode)
    for name, value in (switches or {}).items():
        eng.set_debug_switch(name, value)
    if gd:
        eng.set_decimation(c["round_iters"], c["max_rounds"], c["freeze_llr"])
    return eng


def _decode(c, mode=None):
    eng = _engine(c, True, mode)
    try:
        with launch_util.launch_log() as log:
            out = eng.decode_batch(c["synd"])
    finally:
        eng.close()
    return out, log


def _assert_gd(log, name):
    launch_util.assert_resolved(log)
    assert launch_util.of(log, *EDGE_GD) == [name] and log[name] == 1, f"expected exactly {name}, once; the log has {sorted(log)}"
    launch_util.assert_ran(log, "edge_prior_kernel")
    launch_util.assert_not_ran(log, *PLAIN_BP)


def _gd_kernel_name(h):
    h = sp.csr_matrix(h)
    m, max_row, max_col = h.shape[0], int(np.diff(h.indptr).max()), int(np.asarray(h.sum(axis=0)).max())
    if max_row <= 4 and max_col <= 2:
        return f"bp_edge_gd_kernel<{lu.edge_rounds(m)}>"
    dc = 3 if max_col <= 3 else 4
    return f"bp_edge8_gd_kernel<{lu.edge8_rounds(m, dc)}, {dc}>"


def _assert_shows_all_three(want, rounds, what):
    early, late, never = gu.shows(want, rounds)
    print(f"{what}: {early} rows solved in round 0, {late} after a decimation, {never} walk every round")
    assert early > 0, f"{what}: no row is solved in round 0"
    assert late > 0, f"{what}: no row is solved after a decimation"
    assert never > 0, f"{what}: no row walks every round"


# ---- 1. every instantiation of both ladders once -------------------------------------------------------------------------------------------------
_LADDER = [c for c in lu.EDGE_CASES if c.id.endswith("-percol") and c.build["m"] % 16 == 0] + \
          [c for c in lu.EDGE8_CASES if c.id.endswith("-percol") and c.build["m"] % 8 == 0 and c.build["m"] > 8]
LADDER_T, LADDER_R, LADDER_SEED = 3, 6, 77
# The rate of the BSC errors the syndromes of a ladder case are drawn from (fu.bsc_syndromes(h, 70, rate, LADDER_SEED)), picked per case on
# the CPU so that the restatement shows all three kinds of row.  None: no rate tried gives all three -- the case keeps the ladder's own
# syndromes and asserts "some row converges, some row walks every round".
# Tried: 0.001 .. 0.2 in thirteen steps.  The random members of the bp_edge family (columns of at most two entries) and the larger bp_edge8
# ones rarely gain a row from five decimations of three iterations; every one of their rows that walks is still compared bit for bit.
LADDER_RATE = {
    "edge-R1-m16-percol": 0.08, "edge-R2-m32-percol": None, "edge-R3-m48-percol": 0.05, "edge-R4-m64-percol": None, "edge-R5-m80-percol": None,
    "edge-R6-m96-percol": 0.05, "edge-R7-m112-percol": None, "edge-R8-m128-percol": None, "edge-R9-m144-percol": None, "edge-R10-m160-percol": None,
    "edge-R11-m176-percol": None, "edge-R12-m192-percol": None, "edge-R13-m208-percol": None, "edge-R14-m224-percol": None, "edge-R15-m240-percol": 0.005,
    "edge-R16-m256-percol": None,
    "edge8-DC3-R2-m16-percol": 0.08, "edge8-DC3-R3-m24-percol": 0.03, "edge8-DC3-R4-m32-percol": None, "edge8-DC3-R5-m40-percol": None,
    "edge8-DC3-R6-m48-percol": 0.02, "edge8-DC3-R7-m56-percol": 0.04, "edge8-DC3-R8-m64-percol": 0.01, "edge8-DC3-R9-m72-percol": None,
    "edge8-DC3-R10-m80-percol": None, "edge8-DC3-R12-m96-percol": None,
    "edge8-DC4-R2-m16-percol": 0.12, "edge8-DC4-R3-m24-percol": 0.08, "edge8-DC4-R4-m32-percol": 0.04, "edge8-DC4-R5-m40-percol": 0.02,
    "edge8-DC4-R6-m48-percol": 0.08, "edge8-DC4-R7-m56-percol": None, "edge8-DC4-R8-m64-percol": 0.08, "edge8-DC4-R9-m72-percol": 0.04,
}
KEEPS_THE_LADDERS_SYNDROMES = tuple(k for k, v in LADDER_RATE.items() if v is None)


def test_the_ladder_names_every_instantiation_once():
    names = sorted(_gd_kernel_name(lu.inputs(c.id)[0]) for c in _LADDER)
    want = sorted([f"bp_edge_gd_kernel<{r}>" for r in range(1, 17)] + [f"bp_edge8_gd_kernel<{r}, {dc}>" for dc in (3, 4) for r in lu.EDGE8_ROUNDS[dc]])
    assert names == want and len(names) == 34
    assert sorted(LADDER_RATE) == sorted(c.id for c in _LADDER)
    assert len(KEEPS_THE_LADDERS_SYNDROMES) == 18, "16 of the 34 cases show all three kinds of row; the 18 named above keep the ladder's syndromes"


@pytest.mark.parametrize("case", _LADDER, ids=[c.id for c in _LADDER])
def test_every_instantiation(case):
    """T = 3, R = 6, C = 25, B = 70, the ladder's per-column priors (one column at p = 0.7, one at 0.5)."""
    h, probs, synd = lu.inputs(case.id)
    rate = LADDER_RATE[case.id]
    synd = np.ascontiguousarray(synd[:70]) if rate is None else fu.bsc_syndromes(h, 70, rate, LADDER_SEED)
    c = dict(h=h, probs=np.array(probs), synd=synd, alpha=case.alpha, round_iters=LADDER_T, max_rounds=LADDER_R, freeze_llr=25.0)
    want = gu.bpgd_restatement(h, c["probs"], synd, LADDER_T, LADDER_R, 25.0, case.alpha, details=True)
    if rate is None:
        print(f"{case.id}: the ladder's syndromes: {gu.shows(want, LADDER_R)}")
        assert want[3].any() and not want[3].all(), f"{case.id}: some row converges, some row walks every round"
    else:
        _assert_shows_all_three(want, LADDER_R, f"{case.id} at rate {rate}")
    assert (want[4]["frozen"] >= 0).any()
    eng = _engine(c, mode=case.mode)
    try:
        assert eng.decimation_route(70) == ("bp_edge" if case in lu.EDGE_CASES else "bp_edge8")
        with launch_util.launch_log() as log:
            got = eng.decode_batch(synd)
    finally:
        eng.close()
    _same(got, want, case.id)
    _assert_gd(log, _gd_kernel_name(h))


def test_the_route_without_a_handle_is_the_librarys():
    """ldpc_amd.bpgd_decoder.lane_edge_route restates plan_edge / plan_edge8: on every ladder case and on the cases just outside them."""
    from ldpc_amd.bpgd_decoder import lane_edge_route
    for case in _LADDER + lu.OUTSIDE_CASES:
        h, probs, _ = lu.inputs(case.id)
        eng = _engine(dict(h=h, probs=np.array(probs), alpha=0.625, round_iters=2, max_rounds=2, freeze_llr=25.0))
        try:
            assert eng.decimation_route(70) == lane_edge_route(h), case.id
        finally:
            eng.close()


# ---- 2. the three codes of the lane = edge tests, B = 70 and B = 300 (one wavefront per syndrome: launch_edge gives every row of a batch below
# ----    256 x the resident wavefronts per CU its own workgroup; the work pools are section 2b's), syndrome bytes 2 and 3 -------------------------
_EDGE_NAMES = {"surface5": "bp_edge_gd_kernel<1>", "bb144": "bp_edge8_gd_kernel<9, 3>", "hgp_hamming3": "bp_edge8_gd_kernel<3, 4>"}
EDGE_T, EDGE_R = 3, 8


def _edge_case(code, alpha=0.625, freeze=25.0):
    """mem_bp_util.edge_case's first 300 syndromes with a byte 2 in row 3, a byte 3 in row 9, a byte 2 in row 64 and in row 290 (beyond the
    B = 70 batches)."""
    c = mu.edge_case(code)
    synd = np.ascontiguousarray(c["synd"][:300]).copy()
    m = synd.shape[1]
    synd[3, 5 % m], synd[9, 0], synd[64, m - 1], synd[290, 1] = 2, 3, 2, 2
    return dict(h=c["h"], probs=c["probs"], synd=synd, alpha=alpha, round_iters=EDGE_T, max_rounds=EDGE_R, freeze_llr=freeze)


def _rows(c, want, rows):
    """All 300 rows, or a B = 70 batch (64 + 6: a ragged second tile of work) picked on the RESTATEMENT's output: up to three rows of each
    kind _assert_shows_all_three asks for and the rows with a syndrome byte > 1, then the first rows until there are 70, ascending."""
    if rows == len(c["synd"]):
        return c, want
    sr = want[4]["solved_round"]
    kinds = (sr == 0, sr > 0, ~want[3], (c["synd"] > 1).any(axis=1) & (np.arange(len(sr)) < 70))
    picked = sorted({int(i) for k in kinds for i in np.flatnonzero(k)[:3]})
    picked = np.array(sorted(picked + [i for i in range(len(sr)) if i not in picked][:rows - len(picked)]))
    return dict(c, synd=np.ascontiguousarray(c["synd"][picked])), tuple(x[picked] for x in want[:4]) + ({k: v[picked] for k, v in want[4].items()},)


def _ordinary(c, want):
    """The rows of a batch whose syndrome is bits only (what the decoder classes are given)."""
    keep = (c["synd"] <= 1).all(axis=1)
    return dict(c, synd=np.ascontiguousarray(c["synd"][keep])), tuple(x[keep] for x in want[:4]) + ({k: v[keep] for k, v in want[4].items()},)


@pytest.mark.parametrize("rows", [70, 300])
@pytest.mark.parametrize("code", list(_EDGE_NAMES))
def test_edge_kernels(code, rows):
    full = _edge_case(code)
    c, want = _rows(full, gu.expected(f"edge|{code}", full), rows)
    _assert_shows_all_three(want, EDGE_R, f"{code}/{rows}")
    bad = np.flatnonzero((c["synd"] > 1).any(axis=1))
    assert len(bad) == (4 if rows == 300 else 3) and {int(c["synd"][b].max()) for b in bad} == {2, 3}
    assert not want[3][bad].any() and (want[2][bad] == EDGE_T * EDGE_R).all(), "a syndrome byte > 1 never converges"
    hd = c["h"].toarray().astype(np.int64)
    ok = np.flatnonzero(want[3])
    assert np.array_equal((want[0][ok].astype(np.int64) @ hd.T) & 1, c["synd"][ok]), "a converged row reproduces its syndrome"
    got, log = _decode(c)
    _same(got, want, f"{code}/{rows} rows")
    _assert_gd(log, _EDGE_NAMES[code])


# ---- 2b. work pools: a wavefront that pulls its next syndrome starts from L0 again ---------------------------------------------------------------------
POOL_ROWS = 20011  # (above 256 x 16 workgroups, the most launch_edge starts: wavefronts decode several syndromes each)


def _poisoned(b, n, want_llr=True):
    """Output tensors no decode leaves as they are: 0xFF bytes (decisions and flags are 0 / 1, iteration counts positive), NaN."""
    import torch
    return (torch.full((b, n), 0xFF, dtype=torch.uint8, device="cuda"),
            torch.full((b, n), float("nan"), dtype=torch.float64, device="cuda") if want_llr else None,
            torch.full((b,), -1, dtype=torch.int32, device="cuda"), torch.full((b,), 0xFF, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("chunk,static_pct,want_llr", [(1, 0, True), (8, 50, True), (1, 50, True), (8, 0, True), (8, 50, False)],
                         ids=["chunk1-static0", "chunk8-static50", "chunk1-static50", "chunk8-static0", "chunk8-static50-nollr"])
@pytest.mark.parametrize("code", list(_EDGE_NAMES))
def test_work_pools(code, chunk, static_pct, want_llr):
    """20 011 rows drawn by index from a code's 300 (neighbours of the batch are 37 rows apart in the case): static shares of none and half
    of the batch, pulls of 1 and 8 from the pooled counters, into poisoned outputs.  Rows solved in round 0, rows solved after a decimation
    and rows that walk every round follow one another with different frozen columns: a wavefront that kept its predecessor's frozen
    priors, messages or mask -- or loaded them once, before the syndrome loop -- decodes the next row to other bits."""
    import torch
    full = _edge_case(code)
    want_rows = gu.expected(f"edge|{code}", full)
    idx = (np.arange(POOL_ROWS, dtype=np.int64) * 37) % len(full["synd"])
    want = tuple(x[idx] for x in want_rows[:4]) + ({k: v[idx] for k, v in want_rows[4].items()},)
    _assert_shows_all_three(want, EDGE_R, f"{code} x {POOL_ROWS}")
    sr, chosen = want[4]["solved_round"], want[4]["frozen"]
    after_walker = np.flatnonzero(~want[3][:-1] & (sr[1:] == 0))
    after_late = np.flatnonzero((sr[:-1] > 0) & ~want[3][1:])
    assert len(after_walker) and len(after_late), "a row solved in round 0 follows a row that froze a column in every round, and a walker follows a row solved late"
    assert (chosen[:-1, 0] != chosen[1:, 0]).any(), "neighbouring rows freeze different columns"
    assert not np.isnan(want[1]).any() and want[2].min() >= 1, "the poison must differ from every expected value"
    synd = torch.as_tensor(np.ascontiguousarray(full["synd"][idx]), device="cuda")
    eng = _engine(full, mode=6, switches={"EDGE_CHUNK": chunk, "EDGE_STATIC_PCT": static_pct})
    try:
        out = _poisoned(POOL_ROWS, full["h"].shape[1], want_llr)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(synd, want_llr=want_llr, out=out)
            torch.cuda.synchronize()
    finally:
        eng.close()
    assert all(g is o for g, o in zip(got, out))
    dec, llr, it, cv = (None if x is None else x.cpu().numpy() for x in got)
    if not want_llr:
        assert llr is None
        llr = want[1]
    assert set(np.unique(cv).tolist()) <= {0, 1}, "converge flags that were never written"
    _same((dec, llr, it, cv), want, f"{code} x {POOL_ROWS} rows, chunk {chunk}, static {static_pct} %")
    _assert_gd(log, _EDGE_NAMES[code])


# ---- 3. one round is the plain decode; off, on, off; new channel probabilities; the adaptive alpha ------------------------------------------------------
@pytest.mark.parametrize("code", ["surface5", "bb144"])
def test_one_round_is_the_plain_decode_of_the_same_handle(code):
    full = _edge_case(code)
    c = dict(full, synd=np.ascontiguousarray(full["synd"][:70]), round_iters=12, max_rounds=1)
    want = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], 12, c["alpha"], np.float64)
    assert want[3].any() and not want[3].all()
    eng = _engine(c, gd=False, max_iter=12)
    try:
        plain = eng.decode_batch(c["synd"])
        eng.set_decimation(12, 1, 25.0)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
    finally:
        eng.close()
    _same(plain, want, "the plain decode against the plain restatement")
    _same(got, want, "R = 1 against the plain restatement")
    _same(got, (np.asarray(plain[0]), np.asarray(plain[1]), np.asarray(plain[2]), np.asarray(plain[3], bool)), "R = 1 against the plain decode")
    _assert_gd(log, _EDGE_NAMES[code])


def test_off_on_off_again():
    full = _edge_case("bb144")
    c, want = _rows(full, gu.expected("edge|bb144", full), 70)
    plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], 12, c["alpha"], np.float64)
    eng = _engine(c, gd=False, max_iter=12)
    try:
        assert eng.decimation is None
        with launch_util.launch_log() as log0:
            got = eng.decode_batch(c["synd"])
        _same(got, plain, "before the decimation")
        launch_util.assert_not_ran(log0, *EDGE_GD)
        eng.set_decimation(EDGE_T, EDGE_R, 25.0)
        assert eng.decimation == (EDGE_T, EDGE_R, 25.0) and eng.decimation_route(70) == "bp_edge8"
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, want, "with the decimation")
        _assert_gd(log, "bp_edge8_gd_kernel<9, 3>")
        eng.set_decimation(None)
        assert eng.decimation is None
        with pytest.raises(ValueError, match="guided decimation is not on"):
            eng.decimation_route(70)
        with launch_util.launch_log() as log:
            got = eng.decode_batch(c["synd"])
        _same(got, plain, "decimation off again")
        assert log == log0, f"with the decimation off the handle launches {sorted(log.items())}, before it was ever set {sorted(log0.items())}"
        eng.set_decimation(2, None, np.inf)
        assert eng.decimation == (2, 144, np.inf)
    finally:
        eng.close()


def test_channel_probabilities_set_after_the_decimation_are_followed():
    full = _edge_case("bb144")
    c = dict(full, synd=np.ascontiguousarray(full["synd"][:70]))
    other = dict(c, probs=c["probs"] * np.random.default_rng(11).uniform(0.5, 1.5, size=len(c["probs"])))
    want = gu.expected("edge|bb144|other priors|70", other)
    _assert_shows_all_three(want, EDGE_R, "bb144 with other priors")
    assert not bits_equal(want[1], gu.expected("edge|bb144", full)[1][:70])
    eng = _engine(c)
    try:
        eng.decode_batch(c["synd"])
        eng.set_channel(other["probs"])
        _same(eng.decode_batch(c["synd"]), want, "after set_channel")
    finally:
        eng.close()


@pytest.mark.parametrize("code", ["surface5", "hgp_hamming3"])
def test_scaling_factor_zero_uses_the_total_iteration_count(code):
    """ms_scaling_factor 0: alpha = 1 - 2^-it with the row's TOTAL it -- rows solved in round 1 and later have run under alphas a count
    restarted every round would not produce."""
    full = _edge_case(code, alpha=0.0)
    c, want = _rows(full, gu.expected(f"edge|{code}|alpha0", full), 70)
    early, late, never = gu.shows(want, EDGE_R)
    assert late > 0 and never > 0 and (want[2][want[3]] > EDGE_T).any(), f"{code}: {early}, {late}, {never}"
    got, log = _decode(c)
    _same(got, want, f"{code}, alpha 0")
    _assert_gd(log, _EDGE_NAMES[code])


# ---- 4. ties, nothing left to freeze, infinite priors, freeze_llr = inf ---------------------------------------------------------------------------------
def test_ties_and_all_frozen():
    c = gu.tie_case()
    want = gu.expected("tie", c)
    n = c["h"].shape[1]
    assert want[4]["frozen"][0].tolist() == list(range(n)) + [-1] and (want[2] == c["max_rounds"] * c["round_iters"]).all()
    got, log = _decode(c)
    _same(got, want, "rep_code(5), ties")
    _assert_gd(log, "bp_edge_gd_kernel<1>")


@pytest.mark.parametrize("code,alpha,freeze", [("hamming3", 0.625, 25.0), ("rep5", 0.0, 25.0), ("hamming3", 1.25, np.inf)])
def test_infinite_priors_and_an_infinite_freeze_value(code, alpha, freeze):
    """p = 0, 1, 0.5, 1e-300: the columns with infinite log-ratios are never chosen (column 0 among them: the phantom lanes' column in
    bp_edge's tables); C = +inf at alpha 1.25: NaN posteriors, decided 0."""
    c = gu.edge_channel_case(code, alpha, freeze)
    want = gu.expected(f"edge_channel|{code}|{alpha}|{freeze}", c)
    assert want[3].any() and not want[3].all() and (want[4]["frozen"] >= 0).any()
    if np.isinf(freeze):
        assert np.isnan(want[1]).any()
    got, log = _decode(c)
    _same(got, want, f"{code}, alpha {alpha}, C = {freeze}")
    _assert_gd(log, "bp_edge8_gd_kernel<2, 3>" if code == "hamming3" else "bp_edge_gd_kernel<1>")


# ---- 5. the decoder classes, BP + OSD-0, the detector-error-model loop ------------------------------------------------------------------------------
def test_bpgd_decoder_and_the_bp_decoder_property():
    from ldpc_amd.bp_decoder import BpDecoder
    from ldpc_amd.bpgd_decoder import BpgdDecoder
    full = _edge_case("bb144")
    c, want = _ordinary(*_rows(full, gu.expected("edge|bb144", full), 70))
    assert c["synd"].any(axis=1).all(), "no all-zero row: nothing takes the host shortcut"
    _assert_shows_all_three(want, EDGE_R, "bb144, the rows without a byte > 1")
    d = BpgdDecoder(c["h"], channel_probs=c["probs"], round_iters=EDGE_T, max_rounds=EDGE_R, freeze_llr=25.0, ms_scaling_factor=c["alpha"])
    assert d.route == "bp_edge8"
    with launch_util.launch_log() as log:
        dec = d.decode_batch(c["synd"])
    _same((dec, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), want, "BpgdDecoder.decode_batch")
    _assert_gd(log, "bp_edge8_gd_kernel<9, 3>")
    for row in (int(np.flatnonzero(~want[3])[0]), int(np.flatnonzero(want[4]["solved_round"] > 0)[0])):
        out = d.decode(c["synd"][row])
        _same((out[None, :], d.log_prob_ratios[None, :], np.array([d.iter]), np.array([d.converge])), tuple(x[row:row + 1] for x in want[:4]), f"BpgdDecoder.decode row {row}")
    d2 = BpgdDecoder(c["h"], error_rate=0.2, round_iters=EDGE_T, max_rounds=EDGE_R, ms_scaling_factor=c["alpha"])
    d2.update_channel_probs(c["probs"])
    dec = d2.decode_batch(c["synd"])
    _same((dec, d2.log_prob_ratios_batch, d2.iter_batch, d2.converge_batch), want, "BpgdDecoder after update_channel_probs")
    # BpDecoder.decimation: on, and None switches back to the plain decode
    b = BpDecoder(c["h"], error_channel=list(c["probs"]), max_iter=12, bp_method="minimum_sum", ms_scaling_factor=c["alpha"], input_vector_type="syndrome")
    plain = fu.min_sum_restatement(c["h"], c["probs"], c["synd"], 12, c["alpha"], np.float64)
    dec = b.decode_batch(c["synd"])
    _same((dec, b.log_prob_ratios_batch, b.iter_batch, b.converge_batch), plain, "BpDecoder before")
    b.decimation = dict(round_iters=EDGE_T, max_rounds=EDGE_R)
    assert b.decimation_route == "bp_edge8"
    dec = b.decode_batch(c["synd"])
    _same((dec, b.log_prob_ratios_batch, b.iter_batch, b.converge_batch), want, "BpDecoder.decimation")
    b.decimation = None
    dec = b.decode_batch(c["synd"])
    _same((dec, b.log_prob_ratios_batch, b.iter_batch, b.converge_batch), plain, "BpDecoder after decimation = None")


def test_bposd_osd0_with_the_decimation(oracle_built):
    """Rows with a solution: the restatement's.  Rows without: H x = s, and OSD-0 of the host oracle on the restatement's posteriors."""
    from ldpc_amd.bposd_decoder import BpOsdDecoder
    full = _edge_case("bb144")
    c, want = _ordinary(*_rows(full, gu.expected("edge|bb144", full), 70))  # (a byte > 1 is no syndrome OSD can reproduce)
    dec, llr, it, cv = want[:4]
    orc = oracle_built.BpOracle(c["h"], error_channel=c["probs"], max_iter=12, bp_method="minimum_sum", ms_scaling_factor=c["alpha"])
    expect = dec.copy()
    for b in np.flatnonzero(~cv):
        expect[b] = orc.osdw(c["synd"][b], llr[b], 1, 0)[0]
    d = BpOsdDecoder(c["h"], error_channel=list(c["probs"]), max_iter=12, bp_method="minimum_sum", ms_scaling_factor=c["alpha"], osd_method="osd_0")
    d.decimation = dict(round_iters=EDGE_T, max_rounds=EDGE_R)
    with launch_util.launch_log() as log:
        got = d.decode_batch(c["synd"])
    _same((got, d.log_prob_ratios_batch, d.iter_batch, d.converge_batch), (expect, llr, it, cv), "BpOsdDecoder with the decimation")
    _assert_gd(log, "bp_edge8_gd_kernel<9, 3>")
    hd = c["h"].toarray().astype(np.int64)
    left = np.flatnonzero(~cv)
    assert len(left) and np.array_equal((got[left].astype(np.int64) @ hd.T) & 1, c["synd"][left]), "an OSD row does not satisfy H x = s"
    d.osd_method = "osd_cs"
    d.osd_order = 3
    with pytest.raises(NotImplementedError, match="decimation with osd_method='OSD_CS'"):
        d.decode_batch(c["synd"])


def test_simulate_b8_and_the_monte_carlo_class_with_the_decimation():
    """ring8 x 6 rounds (a bp_edge model), BPGD + OSD-0: both counters equal twin -> decode_b8 -> compare, for chunks 3000 and 64; the
    decode_b8 flags and iteration counts are the restatement's."""
    from ldpc_amd.monte_carlo_simulation import MonteCarloDemSimulation
    from test_dem_sampler_twin import unpack
    from test_gpu_dem_sampler import SEED, engine, model, twin
    check, obs, pri = model("ring8x6")
    gd = dict(round_iters=2, max_rounds=6)
    eng = engine(check, pri, obs)
    try:
        eng.set_osd(1, 0)
        eng.set_decimation(2, 6, 25.0)
        assert eng.decimation_route(3000) == "bp_edge"
        _, dets, true_obs = twin("ring8x6", False, 0)
        with launch_util.launch_log() as log:
            pred, _, iters, conv = eng.decode_b8(np.array(dets), with_osd=True)
        launch_util.assert_ran(log, "bp_edge_gd_kernel<3>")
        launch_util.assert_not_ran(log, *PLAIN_BP)
        synd = unpack(np.array(dets), check.shape[0])
        ref = gu.bpgd_restatement(check, np.clip(pri, 1e-9, 1 - 1e-9), synd, 2, 6, 25.0, 0.625, details=True)
        print(f"ring8x6: {gu.shows(ref, 6)}")
        assert ref[3].any() and (ref[4]["solved_round"] > 0).any()
        ref_iters = np.where(synd.any(axis=1), ref[2], 0)  # (decode_b8: all-zero rows take the shortcut -- converged, 0 iterations)
        assert np.array_equal(np.asarray(conv, bool), ref[3] | ~synd.any(axis=1)) and np.array_equal(np.asarray(iters), ref_iters), \
            "decode_b8 with the decimation: flags or iteration counts"
        want = (int(np.count_nonzero((pred != true_obs).any(axis=1))), int(np.count_nonzero(~np.asarray(conv, bool))))
        print(f"ring8x6 with the decimation + OSD-0: {want[0]} logical failures, {want[1]} rows left without a solution, of 3000")
        for chunk in (3000, 64):
            assert eng.simulate_b8(SEED, 0, 3000, chunk=chunk, with_osd=True) == want, f"chunk {chunk}"
    finally:
        eng.close()
    got = MonteCarloDemSimulation((check, obs, pri), target_run_count=3000, batch_size=1024, seed=SEED, max_iter=12, decimation=gd).run()
    assert (got["fail_count"], got["bp_unconverged_count"]) == want
    # a model beyond the lane = edge kernels is refused at run(), by the library, with the follow-ups named
    from ldpc_amd import _lib
    sim = MonteCarloDemSimulation(model("bb144x3"), target_run_count=64, batch_size=64, seed=SEED, max_iter=12, decimation=gd)
    with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: neither lane = edge kernel family"):
        sim.run()


# ---- 6. the C ABI: the setter, the refusals, buffers ------------------------------------------------------------------------------------------------
def test_cabi_setter_and_refusals():
    from ldpc_amd import _lib
    c = gu.edge_channel_case("hamming3", 0.625)
    n = c["h"].shape[1]
    eng = _engine(c)
    lib = eng._lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    T, R, F = c["round_iters"], c["max_rounds"], c["freeze_llr"]
    err = lambda: lib.ldpc_hip_last_error()  # noqa: E731
    try:
        # the setter: -1 (LDPC_HIP_ERR_INVALID) with the value named, and what it held stays
        assert lib.ldpc_hip_bp_set_decimation(eng._h, -2, 4, 25.0) == -1 and b"round_iters is -2" in err()
        assert lib.ldpc_hip_bp_set_decimation(eng._h, 3, 0, 25.0) == -1 and b"max_rounds is 0" in err()
        assert lib.ldpc_hip_bp_set_decimation(eng._h, 3, -1, 25.0) == -1 and b"max_rounds is -1" in err()
        assert lib.ldpc_hip_bp_set_decimation(eng._h, 65536, 32768, 25.0) == -1 and b"65536" in err() and b"32768" in err()
        assert lib.ldpc_hip_bp_set_decimation(eng._h, 3, 4, 0.0) == -1 and b"freeze_llr is 0" in err()
        assert lib.ldpc_hip_bp_set_decimation(eng._h, 3, 4, -25.0) == -1 and b"freeze_llr is -25" in err()
        assert lib.ldpc_hip_bp_set_decimation(eng._h, 3, 4, float("nan")) == -1 and b"freeze_llr is" in err() and b"nan" in err().lower()
        assert lib.ldpc_hip_bp_set_decimation(eng._h, 3, 4, float("-inf")) == -1
        assert lib.ldpc_hip_bp_set_decimation(None, 0, 0, 0.0) == -1 and lib.ldpc_hip_bp_get_decimation(None, None, None, None) == -1
        with pytest.raises(ValueError, match="max_rounds is 0"):
            eng.set_decimation(3, 0, 25.0)
        assert eng.decimation == (T, R, F)
        assert lib.ldpc_hip_bp_set_decimation(eng._h, 32768, 32768, float("inf")) == 0 and eng.decimation == (32768, 32768, np.inf), "2^30 iterations fit"
        eng.set_decimation(T, R, F)
        route = C.c_int32(-1)
        assert lib.ldpc_hip_bp_decimation_route(eng._h, 70, None) == -1 and lib.ldpc_hip_bp_decimation_route(eng._h, -1, C.byref(route)) == -1
        assert lib.ldpc_hip_bp_decimation_route(eng._h, 70, C.byref(route)) == 0 and route.value == 2
        # decimation, relay and memory exclude one another, each naming what to switch off
        g, li = np.zeros((1, n)), np.array([3], np.int32)
        assert lib.ldpc_hip_bp_set_memory(eng._h, vp(np.zeros(n))) == -4 and b"ldpc_hip_bp_set_decimation(h, 0, 0, 0)" in err()
        assert lib.ldpc_hip_bp_set_relay(eng._h, 1, vp(g), vp(li), 1) == -4 and b"ldpc_hip_bp_set_decimation(h, 0, 0, 0)" in err()
        eng.set_decimation(None)
        eng.set_memory(np.zeros(n))
        assert lib.ldpc_hip_bp_set_decimation(eng._h, T, R, F) == -4 and b"ldpc_hip_bp_set_memory(h, NULL)" in err()
        eng.set_memory(None)
        eng.set_relay(g, li, 1)
        assert lib.ldpc_hip_bp_set_decimation(eng._h, T, R, F) == -4 and b"ldpc_hip_bp_set_relay(h, 0" in err()
        eng.set_relay(None)
        assert eng.decimation is None
        eng.set_decimation(T, R, F)
        # the modes, each with its message, nothing launched
        probs_rows = np.tile(np.clip(c["probs"], 0.01, 0.99), (len(c["synd"]), 1))
        with launch_util.launch_log() as log:
            eng.set_params(12, 0, 1.0)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: product-sum"):
                eng.decode_batch(c["synd"])
            eng.set_params(12, 1, 0.625)
            for schedule in ("serial", "serial_relative"):
                eng.set_schedule(schedule)
                with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: the serial schedules"):
                    eng.decode_batch(c["synd"])
            eng.set_schedule("parallel")
            eng.set_random_serial(True, 5)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: the serial schedules"):
                eng.decode_batch(c["synd"])
            eng.set_random_serial(False, 5)
            eng.set_message_dtype("float32")
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: float32 messages"):
                eng.decode_batch(c["synd"])
            eng.set_message_dtype("float64")
            for osd0 in (False, True):
                with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: per-row channel probabilities"):
                    eng.decode_batch(c["synd"], osd0=osd0, channel_probs=probs_rows)
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: soft-syndrome"):
                eng.soft_info_decode_batch(np.ones((2, 3)), np.inf, 2.0)
            for method in (2, 3):
                eng.set_osd(method, 2)
                with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: OSD-E and OSD-CS"):
                    eng.decode_batch(c["synd"], osd=True)
            eng.set_osd(1, 0)
            # the small-code kernel mode 0 (everything per pass): route 0, refused naming the route query and the follow-ups
            eng.set_small_code_kernel(0)
            assert eng.decimation_route(70) == "unavailable"
            with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: neither lane = edge kernel family.*mode 0.*ldpc_hip_bp_decimation_route.*lane = node route.*per-pass route"):
                eng.decode_batch(c["synd"])
            eng.set_small_code_kernel(-1)
        assert not log, f"a refused decode launched something: {sorted(log)}"
        # ... and the handle still decodes
        _same(eng.decode_batch(c["synd"]), gu.expected("edge_channel|hamming3|0.625|25.0", c), "after the refusals")
    finally:
        eng.close()
    # a code neither family takes: route 0 and the same refusal, for BP and for BP + OSD-0; with the decimation off it decodes
    big = fu.irregular_case()
    eng = _engine(dict(big, round_iters=3, max_rounds=4, freeze_llr=25.0))
    try:
        assert eng.decimation_route(130) == "unavailable"
        with launch_util.launch_log() as log:
            for kw in ({}, dict(osd0=True)):
                with pytest.raises(_lib.LdpcHipError, match=r"error -4: guided decimation: neither lane = edge kernel family.*ldpc_hip_bp_decimation_route"):
                    eng.decode_batch(big["synd"], **kw)
        assert not log, f"a refused decode launched something: {sorted(log)}"
        eng.set_decimation(None)
        _same(eng.decode_batch(big["synd"]), fu.expected("irregular", big, np.float64), "irregular600 with the decimation off")
    finally:
        eng.close()


def test_close_frees_every_device_buffer():
    from ldpc_amd import _lib
    held = _lib.load().ldpc_hip_debug_device_buf_bytes
    before = held()
    full = _edge_case("bb144")
    c = dict(full, synd=np.ascontiguousarray(full["synd"][:70]))
    eng = _engine(c, gd=False)
    try:
        eng.decode_batch(c["synd"])
        plain = held()
        eng.set_decimation(EDGE_T, EDGE_R, 25.0)
        eng.decode_batch(c["synd"])
        assert held() == plain, "the decimation adds no device buffer: the slot tables and the per-slot priors are the plain decode's"
        eng.set_osd(1, 0)
        eng.decode_batch(c["synd"], osd=True)
        during = held()
        eng.set_decimation(None)
        assert held() == during
    finally:
        eng.close()
    after = held()
    print(f"guided decimation: device buffer bytes before {before}, with the engine {during}, after close {after}")
    assert during > before and after == before, f"{after - before} bytes of device buffers outlive the handle"
