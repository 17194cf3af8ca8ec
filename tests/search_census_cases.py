"""The case table and the numpy reference of tests/test_gpu_batch_search_census.py (Batch.search_census,
golhip_batch_search_census).  Plain Python, no GPU: tests/test_batch_search_census_cpu.py runs the reference
over the CPU oracle's soups and shows that the cases meet the conditions the GPU test asserts on its
own results; the GPU test compares the kernel's outputs with the same reference.

The references are the ones the suite already holds, imported, not copied: np_cycles
(tests/test_gpu_batch_cycle.py: cycle_start and period by brute force), np_census
(tests/census_matrix_cases.py), box_mask, np_step_plane (tests/test_gpu_batch_plane.py) and np_step_boards
(tests/test_gpu_batch_period.py).  New here: boards_at, board_i(turns[i]) by stepping, and
brent_repeat_turn, the turn at which Brent's snapshots notice a cycle that starts at cycle_start.
"""
import numpy as np

from census_matrix_cases import np_census  # noqa: F401  (re-exported to the two test files)
from test_gpu_batch_cycle import np_cycles  # noqa: F401
from test_gpu_batch_period import LIFE, np_step_boards
from test_gpu_batch_plane import box_mask, np_step_plane

HALF = 0x80000000
TOPOLOGIES = ("torus", "plane")

# (width, height, soup box or None, the seeds, max_turns): width 64 at every height of
# GOLHIP_BOARD_SHAPES -- (W, R) = (1, 1), (1, 2), (1, 4), (2, 4), (4, 4), (8, 4), (16, 4), (16, 8) -- and
# 128 / 256 / 512 x 16: 4, 8 and 16 words per torus row, the row replicated 4, 2, 1 times in the 16 lanes
# (width 64: 2 words, 8 times).  Boxed soups keep numpy cheap; the whole-board 64 x 64 soups run long
# enough for ash_turn >= 512.  Fewer soups where a board has 512 rows.
POSITION = [
    (64, 4, (8, 4), range(0, 12), 600),
    (64, 8, (8, 8), range(100, 112), 600),
    (64, 16, (16, 16), range(200, 212), 1100),
    (64, 32, (16, 16), range(300, 312), 1100),
    (64, 64, (16, 16), range(400, 412), 1100),
    (64, 128, (16, 16), range(500, 510), 1100),
    (64, 256, (16, 16), range(600, 608), 1100),
    (64, 512, (16, 16), range(700, 708), 1100),
    (128, 16, (16, 16), range(800, 812), 1100),
    (256, 16, (16, 16), range(900, 912), 1100),
    (512, 16, (16, 16), range(1000, 1016), 1100),
    (64, 64, None, range(1100, 1104), 3000),
]
POSITION_IDS = [f"{w}x{h}-{'whole' if box is None else 'box%dx%d' % box}" for w, h, box, _, _ in POSITION]
WHOLE_BOARD = POSITION[-1]
WIDTH_512 = POSITION[-2]
# the two cases that are not about the shape, at 64 x 16 with a 16 x 16 box: density 0 (the empty board is
# on its cycle at turn 0: cycle_start == 0, ash_turn == 0) and a max_turns too small for most soups
EMPTY = (64, 16, (16, 16), range(2), 300)
TOO_SHORT = (64, 16, (16, 16), range(200, 212), 12)


def boards_at(cells, rules, turns, plane):
    """board_i(turns[i]) of an (n, h, w) stack of 0/1 boards, board i under rules[i] (a single pair:
    every board under it), by stepping; a board with turns[i] < 0 comes back dead.  Where the live
    cells of all boards and their neighbours lie strictly inside the rectangle and no rule has B0,
    only that window is stepped, as a plane: nothing outside it can be born, on either topology."""
    cur = np.ascontiguousarray(cells, dtype=np.uint8)
    n, h, w = cur.shape
    turns = np.asarray(turns, dtype=np.int64)
    pairs = np.asarray(rules, dtype=np.int32).reshape(-1, 2)
    no_b0 = not (pairs[:, 0] & 1).any()
    out = np.zeros_like(cur)
    last = int(turns.max()) if n else -1
    for t in range(last + 1):
        hit = turns == t
        out[hit] = cur[hit]
        if t == last:
            break
        ys, xs = np.nonzero(cur.any(axis=(0, 2)))[0], np.nonzero(cur.any(axis=(0, 1)))[0]
        if no_b0 and not ys.size:
            continue  # every board is dead and stays dead
        if no_b0 and ys[0] >= 2 and ys[-1] <= h - 3 and xs[0] >= 2 and xs[-1] <= w - 3:
            y0, y1, x0, x1 = int(ys[0]) - 1, int(ys[-1]) + 2, int(xs[0]) - 1, int(xs[-1]) + 2
            nxt = np.zeros_like(cur)
            nxt[:, y0:y1, x0:x1] = np_step_plane(cur[:, y0:y1, x0:x1], rules)
            cur = nxt
        else:
            cur = np_step_plane(cur, rules) if plane else np_step_boards(cur, rules)
    return out


def brent_repeat_turn(cycle_start, period, max_turns):
    """The record's repeat_turn of a soup whose cycle starts at cycle_start with this (minimal) period:
    the least t >= 1 with board(t) == board(s(t)), s(t) = 2^floor(log2 t) - 1 -- the first window whose
    snapshot turn 2^j - 1 is on the cycle and which is long enough (2^j turns) to hold a period -- or -1
    if that is beyond max_turns or there is no cycle."""
    if cycle_start < 0:
        return -1
    j = 0
    while (1 << j) - 1 < cycle_start or period > (1 << j):
        j += 1
    t = (1 << j) - 1 + int(period)
    return t if t <= max_turns else -1


def reference(golhip, cells, rules, max_turns, plane):
    """What search_census must give for these soups, but for the census: (repeat_turn, period,
    cycle_start, ash_turn, the boards at ash_turn), all by numpy and the documented functions."""
    start, period = np_cycles(cells, rules, max_turns, plane)
    rep = np.array([brent_repeat_turn(int(s), int(p), max_turns) for s, p in zip(start, period)], dtype=np.int64)
    start = np.where(rep >= 0, start, -1)
    period = np.where(rep >= 0, period, -1)
    turn = np.array([golhip.search_census_turn(int(r), int(p), int(s)) for r, p, s in zip(rep, period, start)],
                    dtype=np.int64)
    return rep, period, start, turn, boards_at(cells, rules, turn, plane)


def oracle_cells(oracle, w, h, seeds, box, density_q32=HALF):
    """The soups of these seeds from the CPU oracle's generator, the cells outside the box cleared: what
    Batch.init_random and the search kernels seed."""
    cells = np.stack([(oracle.unpack(oracle.init_random(w, h, int(s), density_q32), w) != 0).astype(np.uint8)
                      for s in seeds])
    return cells if box is None else cells * box_mask(w, h, box)[None]


def common_patterns(golhip):
    return [a for v in golhip.common_objects().values() for a in v]


__all__ = ["LIFE", "HALF", "TOPOLOGIES", "POSITION", "POSITION_IDS", "WHOLE_BOARD", "WIDTH_512", "EMPTY", "TOO_SHORT",
           "boards_at", "brent_repeat_turn", "reference", "oracle_cells", "common_patterns", "np_census", "np_cycles",
           "box_mask"]
