"""The properties of the batches that tests/test_gpu_f32_two_pass.py relies on, from the float32 restatement alone (no GPU): how many rows
each forced first pass leaves and in how many tiles, where the pricing of ``stream_first_pass_length`` (csrc/host_handle.h), restated in
tests/f32_two_pass_util.py, cuts them, and what the big schedule gives the second pass's tile list."""
import numpy as np

import f32_two_pass_util as tu
import f32_util as fu


def _tiles(rows):
    return (rows + 63) // 64, rows % 64


def test_standard_schedule_rows_left_by_each_first_pass():
    case, idx, synd, want = fu.standard_schedule()
    assert case["max_iter"] == 16 and len(idx) == 4423 and (len(idx) + 63) // 64 == 70
    left = {k1: tu.rows_left(want, k1, 16) for k1 in (2, 3, 4, 5, 8, 15)}
    print(f"standard schedule: rows still decoding after k1 iterations {left}")
    assert [left[k] for k in (2, 3, 4, 5, 8)] == [4008, 3000, 1942, 936, 309]
    assert [_tiles(left[k])[0] for k in (2, 3, 4, 5, 8)] == [63, 47, 31, 15, 5]
    assert all(_tiles(rows)[1] != 0 for rows in left.values()), "a second pass whose last tile is whole: the valid-lane mask is not exercised"
    assert 0 < left[15] < left[8], "k1 = 15: a second pass of one iteration must still have rows"
    assert not want[3].all(), "no row that never converges: nothing would run to max_iter in the second pass"


def test_pricing_cuts_the_standard_schedule_at_6():
    case, idx, synd, want = fu.standard_schedule()
    hist = tu.histogram(want)
    assert hist.sum() == 4423 and hist[0] == (~want[3]).sum() and hist[17:].sum() == 0
    k1, plain, best = tu.first_pass_length(hist, 16)
    print(f"standard schedule: cut at {k1}, plain {plain:.2f} tile-iterations per tile, cut {best:.2f}")
    assert k1 == 6 and round(plain, 2) == 15.75 and round(best, 2) == 7.70
    assert 2 <= k1 < 16 and tu.rows_left(want, k1, 16) > 0, "the automatic mode would not run a second pass"


def test_converging_schedule_is_cut_at_5_and_ends_at_12():
    case, idx, synd, want = fu.standard_schedule(converging_only=True)
    assert want[3].all() and int(want[2].max()) == 12
    k1, plain, best = tu.first_pass_length(tu.histogram(want), 16)
    print(f"converging schedule: cut at {k1}, plain {plain:.2f}, cut {best:.2f}")
    assert k1 == 5
    assert tu.rows_left(want, 12, 16) == 0 and tu.rows_left(want, 11, 16) > 0, "k1 = 12 must leave the second pass without a row, and no earlier cut"


def test_big_schedule_fills_a_second_chunk_of_the_second_tile_list():
    case, idx, synd, want = tu.big_schedule()
    assert len(tu.BIG_FINISH) == 200 and len(idx) == 199 * 64 + 23 == 12759
    assert np.array_equal(fu.tile_end_iterations(fu.expected("irregular600", case, np.float32), idx, 16), np.array(tu.BIG_FINISH))
    left3, left4 = tu.rows_left(want, 3, 16), tu.rows_left(want, 4, 16)
    print(f"big schedule: {left3} rows after 3 iterations, {left4} after 4")
    assert (left3, _tiles(left3)) == (8270, (130, 14)) and (left4, _tiles(left4)) == (5266, (83, 18))
    assert _tiles(left3)[0] > 64 and _tiles(left4)[0] > 64, "the second pass's tile list has no second chunk of 64"
    # rows of the second pass end at different iterations, so its tiles (whatever rows share one) end apart and its compactions find final tiles
    end = fu.row_end_iterations(want, 16)
    later = end[end > 3]
    assert len(np.unique(later)) >= 5 and (later < 8).sum() > 64 * 8


def test_edge_value_batches_carry_their_special_rows_into_a_second_pass():
    for code, alpha in (("hamming3", 0.625), ("rep5", 0.0)):
        case, idx, synd, want = fu.edge_values_batch(code, alpha)
        assert case["max_iter"] >= 8, "the two-pass decode needs max_iter >= 8"
        invalid = (synd > 1).any(axis=1)
        assert invalid.sum() >= 2 and {2, 3} <= set(np.unique(synd).tolist())
        assert not want[3][invalid].any(), "a row with a syndrome byte > 1 never converges: it is in every second pass"
        left = tu.rows_left(want, 2, case["max_iter"])
        print(f"{code}: {left} of {len(idx)} rows after 2 iterations")
        assert 64 < left < len(idx) and np.isinf(want[1]).any()
