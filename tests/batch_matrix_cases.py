"""The case table of tests/test_gpu_batch_matrix.py: every batch kernel family under every rule functor
at every (W, R) of GOLHIP_BOARD_SHAPES, with the expected values by numpy.  Plain Python, no GPU:
tests/test_batch_matrix_cpu.py checks that the table is complete and that its inputs exercise what
they are there for, tests/test_gpu_batch_matrix.py compares the kernels with it.

Nothing here defines a reference of its own.  The steppers and the definitions are those of the
existing modules (np_step_boards, np_periods, np_step_plane, np_settled, np_run, box_mask, records,
np_cycles); this module only feeds them and caches what they return (read-only arrays).  The search
soups are oracle.init_random's, which tests/test_gpu_batch.py shows to be Batch.init_random's.

Per (shape, rule) the table fixes
  * the step and period boards (step_boards): soups of several densities, a tiled soup and two
    constructed boards in one batch, and the checkpoints t1_of(shape, rule) < t2_of(shape, rule);
  * one or two search calls (search_calls): (seeds, density_q32, max_turns); the first is shared by
    every rule of the shape, so that a kernel run under the wrong rule cannot give the right records.
"""
import functools

import numpy as np

from test_gpu_batch_cycle import np_cycles
from test_gpu_batch_period import (BLINKER, BLOCK, HIGHLIFE, LIFE, SEEDS, STROBE, TABLE_RULE, board_with, np_periods,
                                   np_step_boards, soups)
from test_gpu_batch_plane import box_mask, np_run, np_settled, np_step_plane
from test_gpu_batch_plane import np_periods as np_periods_over
from test_gpu_batch_rules import REPLICATOR
from test_gpu_batch_search import HALF, records
from test_gpu_rules import CATALOGUE

DAYNIGHT = CATALOGUE[1]  # B3678/S34678

# (width, height): one per (W, R), the height decides it; rows of 4 torus words, of 8 (256 x 32) and of 16
# (512 x 128)
SHAPES = [(64, 4), (128, 8), (64, 16), (256, 32), (64, 64), (512, 128), (64, 256), (64, 512)]
SHAPE_IDS = [f"{w}x{h}" for w, h in SHAPES]

RULES = {"life": LIFE, "highlife": HIGHLIFE, "daynight": DAYNIGHT, "seeds": SEEDS, "replicator": REPLICATOR,
         "table": TABLE_RULE}
FORM = {"life": 0, "highlife": 1, "daynight": 1, "seeds": 1, "replicator": 1, "table": 2}  # kernel_form on the torus
NON_LIFE = [name for name in RULES if name != "life"]
MIX = [*RULES.values(), STROBE]  # form 3: one rule per board / per soup, cycled


def rotating_rule(shape):
    """The non-Life rule of the exact pass and of the plane at this shape: the five in turn."""
    return NON_LIFE[SHAPES.index(shape) % len(NON_LIFE)]


def big(shape):
    """The two shapes of 2^16 and 2^15 cells: numpy needs about a millisecond per board and turn
    there, so they take 5 boards instead of 7."""
    return shape[0] * shape[1] >= 1 << 15


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------- the step and period boards
def t1_of(shape, name):
    """37 turns, not a multiple of 4: the remainder loop of a launch runs.  21 for Replicator at the
    64-wide shapes up to 64 rows, whose boards are all dead at turn 32."""
    return 21 if name == "replicator" and max(shape) == 64 else 37


def t2_of(shape, name):
    """150 turns; Replicator's boards are all dead after max(width, height) / 2 turns (the rule is
    linear: the 2^k-th power of its step is the sum of the cell's 8 neighbours 2^k away and itself,
    which cancels once 2^(k + 1) is a multiple of both sides), so at 512 x 128 and 64 x 512 its run
    goes past turn 256 + 2, where those boards settle."""
    return 270 if name == "replicator" and max(shape) == 512 else 150


@functools.lru_cache(maxsize=None)
def step_boards(shape):
    """The boards of a shape, the same under every rule: soups at 0.5 (board 0, the dense one), 0.2,
    0.04 and 0.002 (0.01 where 0.002 of the board is less than a cell), a 64-wide soup tiled over the
    board (under Replicator it is dead at turn 32 and repeats at 64 whatever the board's size), three
    lone cells (dead at once except under the table rule, whose S0 keeps them: the board that
    settles under Seeds) and a blinker beside a block.  The two big shapes leave out the 0.04 soup
    and the blinker."""
    w, h = shape
    i = SHAPES.index(shape)
    densities = [0.5, 0.2, 0.002] if big(shape) else [0.5, 0.2, 0.04, 0.002 if w * h > 4096 else 0.01]
    boards = [soups(1, w, h, 10 * i + j + 3, d)[0] for j, d in enumerate(densities)]
    tile = soups(1, 64, min(h, 64), 77 + i, 0.5)[0]
    boards.append(np.tile(tile, (h // tile.shape[0], w // 64)))
    boards.append(board_with(w, h, (["1"], 0, 3), (["1"], h // 2, 23), (["1"], h - 1, 43)))
    if not big(shape):
        boards.append(board_with(w, h, (BLINKER, 1, 5), (BLOCK, 1, 12)))
    return frozen(np.stack(boards))


@functools.lru_cache(maxsize=None)
def torus_expected(shape, rules):
    """Of step_boards(shape) under `rules` (one pair, or a tuple of one pair per board), by the
    references alone: t1, t2, repeat (t1 and t2 -> repeat_turn array), counts (n, t2), at_t1 and at_t2 (the
    boards), settled (t1 and t2 -> np_settled)."""
    cells = step_boards(shape)
    per_board = isinstance(rules[0], tuple)
    name = None if per_board else next(k for k, v in RULES.items() if v == rules)
    t1, t2 = t1_of(shape, name), t2_of(shape, name)
    repeat, counts, at_t2 = np_periods(cells, rules, t2, at=(t1,))
    at_t1, counts_t1 = np_run(cells, rules, t1, step=np_step_boards)
    assert np.array_equal(counts_t1, counts[:, :t1])  # the two references agree where they overlap
    settled_t2 = np_settled(cells, rules, t2, step=np_step_boards)
    settled = {t1: np.where((settled_t2 >= 0) & (settled_t2 <= t1), settled_t2, -1), t2: settled_t2}
    frozen(at_t1, *settled.values())
    return {"t1": t1, "t2": t2, "repeat": repeat, "counts": counts, "at_t1": at_t1, "at_t2": at_t2, "settled": settled}


def mix_rules(n):
    return tuple(MIX[i % len(MIX)] for i in range(n))


# ---------------------------------------------------------------- the search calls
Q02, Q004, Q0002 = 0x33333333, 0x0A3D70A3, 0x0083126E  # 0.2, 0.04, 0.002


def soup_seeds(shape, n=None):
    n = 16 if n is None else n
    return tuple(range(1000 * SHAPES.index(shape), 1000 * SHAPES.index(shape) + n))


def shared_call(shape):
    """Dense soups for 100 turns: the call every rule of the shape runs.  146 turns at 128 x 8, where
    Replicator's soups are dead at turn 64, repeat at 128 and are retired at 136."""
    return (soup_seeds(shape), HALF, 146 if shape == (128, 8) else 100)


def search_calls(shape, name):
    """[(seeds, density_q32, max_turns)]: the shared dense call, in which soups run to the end alive,
    and the call that retires soups early."""
    w, h = shape
    if name == "replicator":
        # every soup is dead at turn max(w, h) / 2 and repeats at turn max(w, h).  Up to 128 the
        # shared call passes that turn and its retirement (stop_turn 72 and 136), and a call of 24
        # turns ends below the death turn with the soups alive; from 256 on the shared call is the
        # one below and the second one passes the repeat turn and its retirement, with 4 soups
        # where that takes 530 turns
        repeat = max(w, h)
        if repeat <= 128:
            return [shared_call(shape), (soup_seeds(shape), HALF, 24)]
        retire = 32 * ((repeat - 1) // 32) + 40
        return [shared_call(shape), (soup_seeds(shape, 4 if repeat == 512 else None), HALF, retire + 10)]
    if name == "seeds":  # dense Seeds soups never repeat: the repeats come from 0.002 (64 x 4: half a cell, so 0.04)
        sparse = Q004 if shape == (64, 4) else Q0002
    elif name == "table":  # lone cells survive: at 0.04 the larger boards burn on, at 0.002 they freeze
        sparse = Q004 if w * h <= 4096 and shape != (256, 32) else Q0002
    else:
        sparse = Q004
    return [shared_call(shape), (soup_seeds(shape), sparse, 120)]


@functools.lru_cache(maxsize=None)
def soup_cells(shape, seeds, density_q32, box=None):
    """The soups as Batch.init_random makes them, from the CPU oracle; outside `box` cleared."""
    import oracle

    oracle.build()
    w, h = shape
    cells = np.stack([(oracle.unpack(oracle.init_random(w, h, int(s), density_q32), w) != 0).astype(np.uint8)
                      for s in seeds])
    if box is not None:
        cells = cells * box_mask(w, h, box)[None]
    return frozen(cells)


@functools.lru_cache(maxsize=None)
def search_expected(shape, rules, call, plane=False, box=None):
    """The records of a call under `rules` (one pair, or a tuple of one pair per soup)."""
    seeds, density_q32, max_turns = call
    cells = soup_cells(shape, seeds, density_q32, box)
    step = np_step_plane if plane else np_step_boards
    repeat, counts, _ = np_periods_over(cells, rules, max_turns, step=step)
    want = records(repeat[max_turns], counts, max_turns)
    frozen(*want.values())
    return want


@functools.lru_cache(maxsize=None)
def cycle_expected(shape, rules, call, plane=False, box=None):
    """(cycle_start, period) of a call's soups by the brute force of tests/test_gpu_batch_cycle.py."""
    seeds, density_q32, max_turns = call
    return frozen(*np_cycles(soup_cells(shape, seeds, density_q32, box), rules, max_turns, plane))


# ---------------------------------------------------------------- the plane
PLANE_T1, PLANE_T2 = 37, 100
BOXED_TORUS_SHAPES = [(128, 8), (256, 32), (512, 128)]  # 4, 8 and 16 torus words wide


def plane_box(shape):
    """A soup box smaller than the board, off the word boundaries where the board allows."""
    w, h = shape
    return (min(w, 64) - 14, max(h // 2, 3))


def plane_call(shape):
    """On a plane soups die out or freeze sooner than on the torus: the 0.2 soups for 100 turns."""
    return (soup_seeds(shape), Q02, 100)


@functools.lru_cache(maxsize=None)
def plane_expected(shape):
    """step_boards(shape) on the plane under the shape's rotating rule."""
    cells, rule = step_boards(shape), RULES[rotating_rule(shape)]
    repeat, counts, at_t2 = np_periods_over(cells, rule, PLANE_T2, at=(PLANE_T1,))
    settled_t2 = np_settled(cells, rule, PLANE_T2)
    settled = {PLANE_T1: np.where((settled_t2 >= 0) & (settled_t2 <= PLANE_T1), settled_t2, -1), PLANE_T2: settled_t2}
    torus = torus_expected(shape, rule)
    frozen(*settled.values())
    return {"repeat": repeat, "counts": counts, "at_t2": at_t2, "settled": settled,
            "differs_from_torus": not np.array_equal(counts, torus["counts"][:, :PLANE_T2])}
