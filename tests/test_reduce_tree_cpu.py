"""reduce_tree.py (the numpy restatement of csrc/wave_ops.h's summation order) against a two-tile case
worked out by hand, chosen so that another order gives other bits."""
import numpy as np

import reduce_tree as RT

BIG = 2.0 ** 24  # in fp32 BIG + 1 == BIG, BIG + 2 is exact, BIG + 3 rounds (a tie, to even) to BIG + 4


def _terms():
    """One image of 16 x 65: tile 0 is columns 0 .. 63, tile 1 is column 64."""
    t = np.zeros((1, 16, 65), dtype=np.float32)
    t[0, 0, 0] = BIG
    t[0, 0, 1:5] = 1.0
    t[0, 2, 4] = 1.0
    t[0, 0, 64] = 0.5
    t[0, 5, 64] = 0.25
    return t


def test_quad_threads_by_hand():
    """conf_loss.hip's map. Thread 0 owns (0, 0 .. 3): ((BIG + 1) + 1) + 1 = BIG. Thread 1 owns (0, 4) and
    thread 33 owns (2, 4), both in wave 0: the butterfly's first step gives lane 1 the sum 1 + 1 = 2, its
    last step gives lane 0 BIG + 2. Tile 1: thread 0 (wave 0) has 0.5 and thread 80 (wave 1) 0.25."""
    part = RT.tile_partials(_terms(), RT.QUAD)
    assert part.dtype == np.float32 and part.tolist() == [[BIG + 2, 0.75]]
    # lanes 0 and 1 hold the two tiles; (BIG + 2.75) / 2 = 2^23 + 1.375 rounds to 2^23 + 1 in fp32
    assert RT.same_bits(RT.loss(_terms(), 2.0, RT.QUAD), 2.0 ** 23 + 1)


def test_row_threads_by_hand():
    """view_warp.hip's map. Wave 0 owns row 0, one column per lane: lane 0 has BIG, lanes 1 .. 4 have 1.
    Step ^4: lane 0 BIG + 1 = BIG; ^2: lane 0 BIG + 1 = BIG, lane 1 1 + 1 = 2; ^1: lane 0 BIG + 2. Wave 2
    owns row 2: 1. ((BIG + 2) + 0) + 1 is a tie and rounds to BIG + 4. Tile 1: row 0 is wave 0's, row 5
    wave 1's."""
    part = RT.tile_partials(_terms(), RT.ROWS)
    assert part.tolist() == [[BIG + 4, 0.75]]
    assert RT.same_bits(RT.loss(_terms(), 2.0, RT.ROWS), 2.0 ** 23 + 2)  # 2^23 + 2.375 rounds down


def test_second_level_is_lane_strided_in_double():
    """66 tiles of one image: lane 0 adds tiles 0 and 64, lane 1 tiles 1 and 65, before any lane meets
    another. In double 2^53 + 1 == 2^53: tile 0 = 2^53 (as a float32), tile 64 = -2^53, tile 1 = tile 65 = 1
    give (2^53 - 2^53) + (1 + 1) = 2, where tile order would give ((2^53 + 1) .. - 2^53) + 1 = 1. A second
    image is added after the first."""
    part = np.zeros((2, 66), dtype=np.float32)
    part[0, 0], part[0, 64], part[0, 1], part[0, 65] = 2.0 ** 53, -2.0 ** 53, 1.0, 1.0
    part[1, 3] = 4.0
    assert RT.image_sum(part[0]) == 2.0
    assert RT.same_bits(RT.finalize(part, 3.0), 2.0)
