"""Bounded-plane boards and boxed soups on golhip.Batch (golhip_batch_set_topology /
_set_soup_box; the kernels gol_plane_rule, gol_plane_period and gol_plane_search of
csrc/batch_plane.hpp).

A plane of width x height is the torus's cells with every neighbour outside the rectangle dead.
The reference is numpy: np_step_plane is np_step_boards of tests/test_gpu_batch_period.py with the
three-row and three-column sums taken over a zero-padded stack instead of np.roll; np_periods and
np_settled restate the header's definitions over it.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from test_gpu_batch_period import (BLINKER, BLOCK, CUTS, GLIDER, HIGHLIFE, LIFE, SOUP_TURNS, STROBE, TABLE_RULE,
                                   board_with, cells_of, check_periods, np_step_boards, period_of, snapshot_turn,
                                   soups)
from test_gpu_batch_search import FIELDS, HALF, check, records, soup_cells

pytestmark = pytest.mark.gpu


def np_step_plane(cells, rules):
    """One generation of an (n, h, w) stack of 0/1 planes, board i under rules[i] = (birth, survive)
    (a single pair: every board under it): the cells outside count as dead and stay dead."""
    rules = np.asarray(rules, dtype=np.int32).reshape(-1, 2)
    birth, survive = rules[:, 0].reshape(-1, 1, 1), rules[:, 1].reshape(-1, 1, 1)
    p = np.pad(cells, ((0, 0), (1, 1), (1, 1)))
    rows = p[:, :-2, :] + p[:, 1:-1, :] + p[:, 2:, :]
    n = (rows[:, :, :-2] + rows[:, :, 1:-1] + rows[:, :, 2:] - cells).astype(np.int32)
    return np.where(cells == 1, (survive >> n) & 1, (birth >> n) & 1).astype(np.uint8)


def np_periods(cells, rules, turns, at=(), step=np_step_plane):
    """The definition of repeat_turn over `step`: ({turn: repeat_turn array after that many turns} for
    the turns in `at` and for `turns`, the (n, turns) alive counts, the boards after `turns`)."""
    cells = np.ascontiguousarray(cells, dtype=np.uint8)
    n = cells.shape[0]
    repeat = np.full(n, -1, dtype=np.int64)
    counts = np.zeros((n, turns), dtype=np.int64)
    found = {}
    snap, cur = cells, cells
    for t in range(1, turns + 1):
        cur = step(cur, rules)
        counts[:, t - 1] = cur.sum(axis=(1, 2))
        same = (cur == snap).all(axis=(1, 2))
        repeat[(repeat < 0) & same] = t
        if (t + 1) & t == 0:  # t = 2^j - 1: the next window's snapshot
            assert snapshot_turn(t + 1) == t
            snap = cur
        if t in at or t == turns:
            found[t] = repeat.copy()
    for a in (counts, cur, *found.values()):
        a.setflags(write=False)
    return found, counts, cur


def np_settled(cells, rules, turns, step=np_step_plane):
    """settled[i]: the smallest turn t >= 2 with board_i(t) == board_i(t - 2), -1 if none in `turns`."""
    cells = np.ascontiguousarray(cells, dtype=np.uint8)
    settled = np.full(cells.shape[0], -1, dtype=np.int64)
    two_back, one_back = None, cells
    cur = cells
    for t in range(1, turns + 1):
        cur = step(cur, rules)
        if two_back is not None:
            same = (cur == two_back).all(axis=(1, 2))
            settled[(settled < 0) & same] = t
        two_back, one_back = one_back, cur
    return settled


def np_run(cells, rules, turns, step=np_step_plane):
    """(the boards after `turns`, the (n, turns) alive counts)."""
    cur = np.ascontiguousarray(cells, dtype=np.uint8)
    counts = np.zeros((cur.shape[0], turns), dtype=np.int64)
    for t in range(turns):
        cur = step(cur, rules)
        counts[:, t] = cur.sum(axis=(1, 2))
    return cur, counts


def np_records(cells, rules, max_turns, step=np_step_plane):
    ref, counts, _ = np_periods(cells, rules, max_turns, step=step)
    return records(ref[max_turns], counts, max_turns)


def box_mask(w, h, box):
    bw, bh = box
    x0, y0 = (w - bw) // 2, (h - bh) // 2
    mask = np.zeros((h, w), dtype=np.uint8)
    mask[y0:y0 + bh, x0:x0 + bw] = 1
    return mask


# ---------------------------------------------------------------- 1. small exact cases at 16 x 16
def test_a_glider_ends_as_a_block_in_the_corner(golhip):
    """Width 16 puts a seam inside every word.  The glider runs into the south-east corner and leaves
    the block in rows and columns 14..15: (64, 1) on the plane, (127, 64) on the torus."""
    board = board_with(16, 16, (GLIDER, 2, 2))[None]
    ref, counts, end = np_periods(board, LIFE, 130, at=(63, 64))
    assert np.array_equal(end[0], board_with(16, 16, (BLOCK, 14, 14)))
    assert ref[130][0] == 64 and period_of(ref[130])[0] == 1 and ref[63][0] == -1
    with golhip.Batch(16, 16, 1, topology="plane") as b:
        assert b.topology == "plane" and b.kernel_form == 0
        b.load(board * 255)
        b.track_period()
        hist = b.step(63, history=True)
        assert np.array_equal(hist.astype(np.int64), counts[:, :63])
        check_periods(b, ref[63], 63)
        b.step(67)
        check_periods(b, ref[130], 130)
        assert np.array_equal(b.periods()[0], [64]) and np.array_equal(b.periods()[1], [1])
        assert np.array_equal(cells_of(b), end)
        # the same board on the torus
        b.load(board * 255)
        b.set_topology("torus")
        assert b.topology == "torus"
        b.step(130)
        assert np.array_equal(b.periods()[0], [127]) and np.array_equal(b.periods()[1], [64])


def test_patterns_on_the_borders(golhip):
    """A blinker lying along each border, a block in each corner, a full row of ones at the top, in the
    middle and at the bottom, and a full board: every turn's count and the boards after 1..4 and 21
    turns."""
    boards = np.stack([board_with(16, 16, (BLINKER, 0, 6)), board_with(16, 16, (BLINKER, 15, 6)),
                       board_with(16, 16, (["1", "1", "1"], 6, 0)), board_with(16, 16, (["1", "1", "1"], 6, 15)),
                       board_with(16, 16, (BLOCK, 0, 0)), board_with(16, 16, (BLOCK, 0, 14)),
                       board_with(16, 16, (BLOCK, 14, 0)), board_with(16, 16, (BLOCK, 14, 14)),
                       board_with(16, 16, (["1" * 16], 0, 0)), board_with(16, 16, (["1" * 16], 7, 0)),
                       board_with(16, 16, (["1" * 16], 15, 0)), np.ones((16, 16), dtype=np.uint8)])
    torus_end = boards
    for _ in range(21):
        torus_end = np_step_boards(torus_end, LIFE)
    with golhip.Batch(16, 16, boards.shape[0], topology="plane") as b:
        b.load(boards * 255)
        cur, done = boards, 0
        for t in (1, 2, 3, 4, 21):
            want, counts = np_run(cur, LIFE, t - done)
            hist = b.step(t - done, history=True)
            assert np.array_equal(hist.astype(np.int64), counts), t
            bad = np.nonzero((cells_of(b) != want).any(axis=(1, 2)))[0]
            assert bad.size == 0, (t, bad)
            cur, done = want, t
        assert (cur != torus_end).any(axis=(1, 2)).sum() >= 4  # the reference alone: the seams matter here


# ---------------------------------------------------------------- 2. every (W, R) and word width
SHAPES = [(16, 4), (64, 8), (256, 16), (512, 32), (128, 64), (256, 128), (512, 256), (64, 512), (512, 512)]


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_every_shape(golhip, w, h):
    """Soups with live cells on every border, 70 turns (the drift passes 32 and 64) with history:
    the stored boards and every count."""
    n = 6 if w * h <= 1 << 16 else 3
    cells = soups(n, w, h, 3 * w + h)
    assert cells[:, 0].any() and cells[:, -1].any() and cells[:, :, 0].any() and cells[:, :, -1].any()
    end, counts = np_run(cells, LIFE, 70)
    torus = cells
    for _ in range(70):
        torus = np_step_boards(torus, LIFE)
    assert (end != torus).any(axis=(1, 2)).sum() > n // 2  # the reference alone: the plane is not the torus
    with golhip.Batch(w, h, n, topology="plane") as b:
        b.load(cells * 255)
        hist = b.step(70, history=True)
        assert np.array_equal(hist.astype(np.int64), counts)
        assert np.array_equal(cells_of(b), end)
        assert np.array_equal(b.alive_counts().astype(np.int64), counts[:, -1])


@pytest.mark.parametrize("size", [16, 64])
def test_600_turns_in_one_call(golhip, size):
    """The drift passes the 512-bit ring."""
    cells = soups(8, size, size, size)
    end, counts = np_run(cells, LIFE, 600)
    with golhip.Batch(size, size, 8, topology="plane") as b:
        b.load(cells * 255)
        hist = b.step(600, history=True)
        assert np.array_equal(hist.astype(np.int64), counts)
        assert np.array_equal(cells_of(b), end)


@pytest.mark.parametrize("w", [1, 2, 4, 8, 32])
def test_narrow_widths(golhip, w):
    """Widths below a word and of one word: the seam mask has a zero every `w` bits (all zeros at 1)."""
    cells = soups(5, w, 16, w, density=0.6)
    end, counts = np_run(cells, LIFE, 40)
    with golhip.Batch(w, 16, 5, topology="plane") as b:
        b.load(cells * 255)
        hist = b.step(40, history=True)
        assert np.array_equal(hist.astype(np.int64), counts)
        assert np.array_equal(cells_of(b), end)


# ---------------------------------------------------------------- 3. settle and periods
@functools.lru_cache(maxsize=None)
def plane_soup_reference(size, turns):
    cells = soups(32, size, size, 100 + size)
    cells.setflags(write=False)
    ref, counts, end = np_periods(cells, LIFE, turns, at=(turns // 4,))
    settled = {t: np_settled(cells, LIFE, t) for t in (turns // 4, turns)}
    return cells, ref, counts, end, settled


@pytest.mark.parametrize("size,turns", [(16, 400), (64, 1200)])
def test_settle_and_periods(golhip, size, turns):
    cells, ref, counts, end, settled = plane_soup_reference(size, turns)
    # the reference alone: boards that repeat and settle, and at 64 x 64 boards that have not yet
    assert (ref[turns] > 0).any() and (settled[turns] > 0).any()
    assert (ref[turns // 4] < 0).any() and (settled[turns // 4] < 0).any()
    with golhip.Batch(size, size, 32, topology="plane") as b:
        b.load(cells * 255)
        b.track_period()
        b.step(turns // 4)
        check_periods(b, ref[turns // 4], "quarter")
        hist = b.step(turns - turns // 4, history=True)
        assert np.array_equal(hist.astype(np.int64), counts[:, turns // 4:])
        check_periods(b, ref[turns], "end")
        assert np.array_equal(cells_of(b), end)
        b.track_period(False)
        b.load(cells * 255)
        b.track_settle()
        b.step(turns // 4)
        assert np.array_equal(b.settled(), settled[turns // 4])
        b.step(turns - turns // 4)
        assert np.array_equal(b.settled(), settled[turns])
        assert np.array_equal(cells_of(b), end)


# ---------------------------------------------------------------- 4. cuts
def test_the_records_do_not_depend_on_the_cuts(golhip):
    cells = soups(64, 32, 32, 2)
    ref, counts, end = np_periods(cells, LIFE, SOUP_TURNS)
    settled = np_settled(cells, LIFE, SOUP_TURNS)
    assert sum(CUTS) == SOUP_TURNS
    assert (ref[SOUP_TURNS] > 0).any() and (settled > 0).any()
    for cuts in ([SOUP_TURNS], CUTS):
        for tracker in ("period", "settle"):
            with golhip.Batch(32, 32, 64, topology="plane") as b:
                b.load(cells * 255)
                done = 0
                b.track_period() if tracker == "period" else b.track_settle()
                for i, n in enumerate(cuts):
                    hist = b.step(n, history=bool(i & 1))
                    if hist is not None:
                        assert np.array_equal(hist.astype(np.int64), counts[:, done:done + n]), (len(cuts), done)
                    done += n
                if tracker == "period":
                    check_periods(b, ref[SOUP_TURNS], len(cuts))
                else:
                    assert np.array_equal(b.settled(), settled), len(cuts)
                assert np.array_equal(cells_of(b), end)


# ---------------------------------------------------------------- 5. rules
def test_highlife_runs_the_table_form_on_the_plane(golhip):
    cells = soups(16, 64, 32, 41)
    ref, counts, end = np_periods(cells, HIGHLIFE, 200)
    with golhip.Batch(64, 32, 16, rule=HIGHLIFE) as b:
        assert b.kernel_form == 1
        b.set_topology("plane")
        assert b.kernel_form == 2
        b.load(cells * 255)
        b.track_period()
        hist = b.step(200, history=True)
        assert np.array_equal(hist.astype(np.int64), counts)
        check_periods(b, ref[200])
        assert np.array_equal(cells_of(b), end)
        b.track_period(False)  # with a tracker on the topology changes at turn 0 only
        b.set_topology("torus")
        assert b.kernel_form == 1


def test_the_table_rule(golhip):
    cells = soups(16, 64, 32, 43, density=0.2)
    end, counts = np_run(cells, TABLE_RULE, 100)
    settled = np_settled(cells, TABLE_RULE, 100)
    with golhip.Batch(64, 32, 16, rule=TABLE_RULE, topology="plane") as b:
        assert b.kernel_form == 2
        b.load(cells * 255)
        b.track_settle()
        hist = b.step(100, history=True)
        assert np.array_equal(hist.astype(np.int64), counts)
        assert np.array_equal(cells_of(b), end)
        assert np.array_equal(b.settled(), settled)


def test_a_b0_rule_strobes_inside_and_the_outside_stays_dead(golhip):
    """B03/S23 on an empty 16 x 8 plane: every cell is born at turn 1 (the full board: nothing
    outside was born, or the edge cells would count neighbours), then the edges and corners have 5
    and 3 live neighbours: the reference knows what follows."""
    cells = np.zeros((2, 8, 16), dtype=np.uint8)
    cells[1] = soups(1, 16, 8, 5)[0]
    ref, counts, end = np_periods(cells, STROBE, 40, at=(1, 2, 3))
    assert counts[0, 0] == 128 and counts[0, 1] < 128
    with golhip.Batch(16, 8, 2, rule=STROBE, topology="plane") as b:
        assert b.kernel_form == 2
        b.load(cells * 255)
        b.track_period()
        hist = b.step(40, history=True)
        assert np.array_equal(hist.astype(np.int64), counts)
        check_periods(b, ref[40])
        assert np.array_equal(cells_of(b), end)


def test_one_rule_per_board(golhip):
    rules = [LIFE, HIGHLIFE, TABLE_RULE, STROBE] * 4
    cells = soups(16, 64, 64, 47)
    cells[:4] = 0
    ref, counts, end = np_periods(cells, rules, 150, at=(3,))
    with golhip.Batch(64, 64, 16, rules=rules, topology="plane") as b:
        assert b.kernel_form == 3
        b.load(cells * 255)
        b.track_period()
        b.step(3)
        check_periods(b, ref[3], 3)
        hist = b.step(147, history=True)
        assert np.array_equal(hist.astype(np.int64), counts[:, 3:])
        check_periods(b, ref[150], 150)
        assert np.array_equal(cells_of(b), end)


# ---------------------------------------------------------------- 6. search on the plane
def test_search_definition(golhip):
    cells = soup_cells(golhip, 64, 16, np.arange(256))
    want = np_records(cells, LIFE, 200)
    early = int(((want["repeat_turn"] > 0) & (want["stop_turn"] < 200)).sum())
    # the reference alone: both classes hold at least a tenth of the soups
    assert early >= 26 and 256 - early >= 26, early
    with golhip.Batch(64, 16, 3, topology="plane") as b:
        check(b.search(256, seed0=0, max_turns=200), want, "seed0")
        check(b.search(256, seeds=np.arange(256), max_turns=200), want, "seeds")
        perm = np.random.default_rng(5).permutation(256)
        check(b.search(256, seeds=perm, max_turns=200), {k: v[perm] for k, v in want.items()}, "perm")


SEARCH_SHAPES = [(64, 4, 64, HALF, 60), (128, 8, 64, HALF, 200), (64, 32, 32, HALF, 600), (64, 64, 16, HALF, 1100),
                 (256, 128, 16, 0x0A3D70A3, 300), (512, 256, 16, 0x07AE147A, 300)]


@pytest.mark.parametrize("w,h,n,density,max_turns", SEARCH_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SEARCH_SHAPES])
def test_search_every_shape(golhip, w, h, n, density, max_turns):
    seeds = np.arange(n, dtype=np.uint64)
    cells = soup_cells(golhip, w, h, seeds, density)
    want = np_records(cells, LIFE, max_turns)
    # the reference alone: soups that are retired before max_turns, and soups without a repeat
    assert (want["stop_turn"] < max_turns).any() and (want["repeat_turn"] < 0).any(), want["repeat_turn"]
    with golhip.Batch(w, h, 1, topology="plane") as b:
        check(b.search(n, seeds=seeds, density_q32=density, max_turns=max_turns), want)


def test_search_one_rule_per_soup(golhip):
    rng = np.random.default_rng(64)
    rules = [LIFE, HIGHLIFE, TABLE_RULE, STROBE] + [tuple(int(v) for v in rng.integers(0, 512, 2)) for _ in range(60)]
    seed, max_turns = 17, 300
    cells = np.repeat(soup_cells(golhip, 64, 16, [seed]), 64, axis=0)
    want = np_records(cells, rules, max_turns)
    assert len(set(want["repeat_turn"])) >= 4, want["repeat_turn"]
    with golhip.Batch(64, 16, 2, topology="plane") as b:
        got = b.search(64, seeds=[seed] * 64, max_turns=max_turns, rules=rules)
        check(got, want)
        for i in (1, 2, 3):  # and as the batch's uniform rule
            b.set_rule(rules[i])
            one = b.search(1, seeds=[seed], max_turns=max_turns)
            assert one[0] == got[i], (i, one[0], got[i])


def test_search_512x512_against_the_step_route(golhip):
    seeds, max_turns = np.array([5, 6, 7, 8], dtype=np.uint64), 150
    with golhip.Batch(512, 512, 4, topology="plane") as b:
        b.init_random(seeds=seeds, density_q32=0x028F5C28)
        b.track_period()
        counts = b.step(max_turns, history=True)
        repeat_turn, period = b.periods()
        want = records(repeat_turn, counts, max_turns)
        assert np.array_equal(want["period"], period)
        before = b.store()
        check(b.search(4, seeds=seeds, density_q32=0x028F5C28, max_turns=max_turns), want)
        assert np.array_equal(b.store(), before) and b.turn == max_turns


@pytest.mark.parametrize("w,h", [(64, 16), (512, 256)], ids=["1wave", "16waves"])
def test_empty_boards_stop_at_every_remainder(golhip, w, h):
    with golhip.Batch(w, h, 1, topology="plane") as b:
        for max_turns in range(1, 71):
            got = b.search(3, seed0=9, density_q32=0, max_turns=max_turns)
            for name, value in zip(FIELDS, (1, 1, min(max_turns, 40), 0, 0)):
                assert (got[name] == value).all(), (max_turns, name, got[name])


def test_search_leaves_the_handle_as_it_was(golhip):
    cells = soups(5, 64, 64, 23)
    ref, _, end = np_periods(cells, LIFE, 137, at=(37,))
    with golhip.Batch(64, 64, 5, topology="plane", soup_box=(16, 16)) as b:
        b.load(cells * 255)
        b.track_period()
        b.step(37)
        state = (b.store(), b.turn, b.periods(), b.rule_masks, b.kernel_form, b.topology, b.soup_box)
        assert b.search(100, seed0=3, max_turns=200).shape == (100,)
        after = (b.store(), b.turn, b.periods(), b.rule_masks, b.kernel_form, b.topology, b.soup_box)
        assert np.array_equal(after[0], state[0]) and after[1] == state[1] == 37
        assert np.array_equal(after[2][0], state[2][0]) and np.array_equal(after[2][1], state[2][1])
        assert after[3:] == state[3:] == (LIFE, 0, "plane", (16, 16))
        b.step(100)
        check_periods(b, ref[137])
        assert np.array_equal(cells_of(b), end)


# ---------------------------------------------------------------- 7. the box
@pytest.mark.parametrize("w,h,boxes", [(64, 64, [(16, 16), (5, 3), (64, 1), (64, 64)]), (256, 128, [(100, 30)])],
                         ids=["64x64", "256x128"])
def test_init_random_in_a_box(golhip, w, h, boxes):
    seeds = np.arange(7, 13, dtype=np.uint64)
    for density in (HALF, 0x4CCCCCCC):  # both density paths
        full = soup_cells(golhip, w, h, seeds, density)
        with golhip.Batch(w, h, len(seeds)) as b:
            assert b.soup_box is None
            for box in boxes:
                b.set_soup_box(box)
                assert b.soup_box == box
                b.init_random(seeds=seeds, density_q32=density)
                want = full * box_mask(w, h, box)
                assert np.array_equal(cells_of(b), want), (density, box)
                b.init_random(seed0=7, density_q32=density)  # the seed0 path
                assert np.array_equal(cells_of(b), want), (density, box)
            b.set_soup_box((0, 0))
            assert b.soup_box is None
            b.init_random(seeds=seeds, density_q32=density)
            assert np.array_equal(cells_of(b), full)
            b.set_soup_box(boxes[0])
            b.load(full * 255)  # a load ignores the box
            assert np.array_equal(cells_of(b), full)


def test_a_boxed_search(golhip):
    """The standard setting: a 16 x 16 soup in a 64 x 64 plane, seeds 0..63, 1100 turns."""
    seeds, max_turns = np.arange(64, dtype=np.uint64), 1100
    cells = soup_cells(golhip, 64, 64, seeds) * box_mask(64, 64, (16, 16))
    want = np_records(cells, LIFE, max_turns)
    torus = np_records(cells, LIFE, max_turns, step=np_step_boards)
    # the reference alone: nearly every soup repeats, a period above 2 is an oscillator; on the torus
    # gliders circle the board
    assert int((want["repeat_turn"] > 0).sum()) == 62 and want["period"].max() <= 6
    assert (torus["period"] == 256).any()
    with golhip.Batch(64, 64, 64, topology="plane", soup_box=(16, 16)) as b:
        got = b.search(64, seeds=seeds, max_turns=max_turns)
        check(got, want, "plane")
        # the step route shows the boards that were searched
        b.init_random(seeds=seeds)
        assert np.array_equal(cells_of(b), cells)
        b.track_period()
        counts = b.step(max_turns, history=True)
        check(got, records(b.periods()[0], counts, max_turns), "step route")
        # the box on the torus
        b.track_period(False)  # with a tracker on the topology changes at turn 0 only
        b.set_topology("torus")
        check(b.search(64, seeds=seeds, max_turns=max_turns), torus, "torus")
        b.set_rule(HIGHLIFE)  # a boxed torus search of a catalogue rule: the table form, the same records
        check(b.search(64, seeds=seeds, max_turns=300), np_records(cells, HIGHLIFE, 300, step=np_step_boards), "highlife")


# ---------------------------------------------------------------- 8. nothing else moved
def test_a_torus_by_any_route_is_the_default_batch(golhip):
    cells = soups(8, 64, 64, 77)
    seeds = np.arange(32, dtype=np.uint64)
    results = []
    for route in ("default", "explicit", "switched"):
        kwargs = {"topology": "torus"} if route == "explicit" else {}
        with golhip.Batch(64, 64, 8, **kwargs) as b:
            if route == "switched":
                b.set_topology("plane")
                b.set_soup_box((8, 8))
                b.set_topology("torus")
                b.set_soup_box(None)
            assert b.topology == "torus" and b.soup_box is None and b.kernel_form == 0
            b.load(cells * 255)
            b.track_settle()
            hist = b.step(300, history=True)
            out = [b.store(), hist, b.settled()]
            b.track_settle(False)
            b.load(cells * 255)
            b.track_period()
            b.step(300)
            out += [*b.periods(), b.search(32, seeds=seeds, max_turns=300)]
            results.append(out)
    for other in results[1:]:
        for a, c in zip(results[0], other):
            assert np.array_equal(a, c)
    torus = cells
    for _ in range(300):
        torus = np_step_boards(torus, LIFE)
    assert np.array_equal((results[0][0] != 0).astype(np.uint8), torus)


# ---------------------------------------------------------------- 9. errors and state
def test_errors_and_state(golhip):
    lib = golhip.load_library()
    cells = soups(3, 64, 32, 3)
    with pytest.raises(golhip.GolHipError) as ei:
        golhip.Batch(64, 32, 3, topology="klein")
    assert ei.value.code == golhip.ERR_ARG
    with pytest.raises(golhip.GolHipError) as ei:
        golhip.Batch(64, 32, 3, soup_box=(65, 1))
    assert ei.value.code == golhip.ERR_ARG
    with golhip.Batch(64, 32, 3) as b:
        b.load(cells * 255)
        b.set_topology("plane")
        b.set_soup_box((10, 7))
        b.step(4)

        def state():
            return (b.store().tobytes(), b.turn, b.topology, b.soup_box, b.kernel_form, b.rule_masks)

        before = state()
        for value in (-1, 2, 7):
            assert lib.golhip_batch_set_topology(b._h, value) == golhip.ERR_ARG
            assert "topology" in lib.golhip_batch_last_error(b._h).decode()
            assert state() == before
        for box in ((0, 5), (5, 0), (65, 1), (1, 33), (-1, -1), (64, 33)):
            with pytest.raises(golhip.GolHipError) as ei:
                b.set_soup_box(box)
            assert ei.value.code == golhip.ERR_ARG and "box" in str(ei.value), box
            assert state() == before
        for box in ((64, 32), (1, 1), (10, 7)):
            b.set_soup_box(box)
            assert b.soup_box == box
        # without tracking the topology changes at any turn
        b.set_topology("torus")
        b.set_topology("plane")
        assert state() == before
        # with tracking on: at turn 0 and after a load only
        for track in (b.track_settle, b.track_period):
            b.load(cells * 255)
            track()
            b.set_topology("torus")  # turn 0: allowed
            b.set_topology("plane")
            b.step(2)
            before = state()
            with pytest.raises(golhip.GolHipError) as ei:
                b.set_topology("torus")
            assert ei.value.code == golhip.ERR_STATE and "turn 0" in str(ei.value)
            assert state() == before
            b.set_topology("plane")  # the current value: no change
            b.load(cells * 255)  # after a load: allowed, and the load keeps the topology
            assert b.topology == "plane"
            b.set_topology("torus")
            b.set_topology("plane")
            track(False)
        # the handle still works
        want, _ = np_run(cells, LIFE, 10)
        b.step(10)
        assert np.array_equal(cells_of(b), want)
