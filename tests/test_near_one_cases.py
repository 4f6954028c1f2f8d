"""The cases of tests/near_one_util.py, checked without a GPU: the census of a plain NumPy restatement shows that every case reaches the paths of
the near-1 parking it is there for -- nothing parked, under / exactly at / past the capacity, dead lanes with near-1 arguments beside live lanes
without, the generic routine in some iterations and the parking path in others -- that no argument is so close to a threshold that the float64
classifier could disagree with the device, and that the shapes stay as small as the issue of this test set them."""
import numpy as np
import pytest

import near_one_util as nu

LANE_IMPLS = ("check_row", "bit_messages")


def _ids(cases):
    return [c.id for c in cases]


def test_slot_counts_come_from_the_headers():
    cap = nu.slot_counts()
    assert set(cap) == {"check_row", "bit_messages", "wave"} and all(8 <= v <= 64 for v in cap.values())
    # the cases below are laid out for these capacities: another value needs other lane counts (8 x 6, 16 x 3, 64 listed entries)
    assert (cap["check_row"], cap["bit_messages"], cap["wave"]) == (48, 48, 64)


def test_labels_of():
    assert nu.labels_of([0, 0], 48) == {"zero"} and nu.labels_of([9, 0, 9], 48) == {"under"} and nu.labels_of([8] * 6, 48) == {"at"}
    assert nu.labels_of([64, 64], 48) == {"over_first"} and nu.labels_of([9] * 6, 48) == {"park_then_over"}
    assert nu.labels_of([64, 8], 48) == {"over_first"} and nu.labels_of([40, 24], 64) == {"at"} and nu.labels_of([64, 2], 64) == {"park_then_over"}


@pytest.mark.parametrize("case", nu.CASES, ids=_ids(nu.CASES))
def test_shapes(case):
    code, synd = case.code(), case.synd()
    m, n = code.h.shape
    assert m <= 24 and n <= 120 and case.max_iter <= 6
    assert len(synd) == 128 or 64 < len(synd) < 128
    assert len(set(np.round(code.probs, 12))) > 3, "non-uniform priors"
    assert synd.shape[1] == m and len(code.probs) == n and (np.asarray(code.h.sum(axis=0)).ravel() >= 1).all()


@pytest.mark.parametrize("case", [c for c in nu.CASES if c.impl], ids=_ids([c for c in nu.CASES if c.impl]))
def test_census_shows_what_the_case_is_for(case):
    cs = nu.census(case.id)
    print(f"{case.id}: {sorted(cs.labels)}; {int(cs.converge.sum())} of {len(cs.converge)} syndromes converge; {case.kernel}")
    assert cs.borderline == 0, "an argument within 1e-9 of a threshold of the log, or a tanh argument where tanh starts to round to 1"
    missing = set(case.shows) - cs.labels
    assert not missing, f"the census lacks {sorted(missing)}; it has {sorted(cs.labels)}"
    assert cs.converge.any() and not cs.converge.all(), "dead lanes beside live lanes"
    assert (cs.iterations[~cs.converge] == case.max_iter).all()


@pytest.mark.parametrize("impl", ("check_row", "bit_messages", "wave"))
def test_every_implementation_sees_every_path(impl):
    """Over its cases, each implementation's census holds every label (the wave kernel lists entries of one syndrome: it has no dead lanes, and
    its first round of 64 slots always fits into 64 slots)."""
    want = {"zero", "under", "at", "park_then_over", "fallback", "fallback_varies"} | ({"over_first", "dead_near"} if impl in LANE_IMPLS else set())
    got = set().union(*(nu.census(c.id).labels for c in nu.CASES if c.impl == impl))
    assert want <= got, sorted(want - got)


def test_phantom_slots_and_a_weight_one_row_take_part():
    """Row weights at and below the instantiation's DR = 8; one fallback case of each family has a row of one entry."""
    weights = np.asarray(nu.BY_ID["var-capacity"].code().h.sum(axis=1)).ravel()
    assert weights.max() == 8 and weights.min() == 2
    for cid in ("var-fallback-weight1-row", "spread-fallback-weight1-row", "wave-fallback-weight1-row"):
        assert np.asarray(nu.BY_ID[cid].code().h.sum(axis=1)).min() == 1
    for cid in ("ring-capacity", "serial-capacity"):
        h = nu.BY_ID[cid].code().h
        assert (np.asarray(h.sum(axis=1)) == 6).all() and (np.asarray(h.sum(axis=0)) == 3).all()


@pytest.mark.parametrize("case", [c for c in nu.CASES if c.impl], ids=_ids([c for c in nu.CASES if c.impl]))
def test_the_restatement_follows_the_oracles_decode(case, oracle_built):
    """The census classifies the decode the kernels run: its iteration counts and converge flags are the oracle's."""
    cs, want = nu.census(case.id), nu.expected(case.id)
    assert np.array_equal(cs.converge, want[3]) and np.array_equal(cs.iterations, want[2])
