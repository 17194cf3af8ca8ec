"""Per-board cycle detection on golhip.Batch (golhip_batch_track_period / _periods, the kernel
gol_batch_period of csrc/batch_period.hpp): Brent's scheme with snapshots at turns 2^j - 1.

The definition, restated here in numpy (np_periods): for t >= 1 let s(t) = 2^floor(log2 t) - 1;
board i repeats at turn t when board_i(t) == board_i(s(t)) over the whole torus; repeat_turn[i] is
the smallest such t among the turns run, period[i] = repeat_turn[i] - s(repeat_turn[i]), both -1
before.  The reference is the numpy stepper below plus that definition, vectorised over boards;
every comparison is exact."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

LIFE = (0x008, 0x00C)
HIGHLIFE = (0x048, 0x00C)    # B36/S23, constant-folded (form 1)
SEEDS = (0x004, 0x000)       # B2/S, constant-folded
TABLE_RULE = (0x108, 0x04D)  # B38/S0236, table form (form 2)
STROBE = (0x009, 0x00C)      # B03/S23: a B0 rule, an empty board strobes with period 2


def np_step_boards(cells, rules):
    """One generation of an (n, h, w) stack of 0/1 tori, board i under rules[i] = (birth, survive)
    (a single pair: every board under it)."""
    rules = np.asarray(rules, dtype=np.int32).reshape(-1, 2)
    birth, survive = rules[:, 0].reshape(-1, 1, 1), rules[:, 1].reshape(-1, 1, 1)
    rows = np.roll(cells, 1, 1) + cells + np.roll(cells, -1, 1)
    n = (np.roll(rows, 1, 2) + rows + np.roll(rows, -1, 2) - cells).astype(np.int32)
    return np.where(cells == 1, (survive >> n) & 1, (birth >> n) & 1).astype(np.uint8)


def snapshot_turn(t):
    """s(t) = 2^floor(log2 t) - 1 for t >= 1."""
    return (1 << (int(t).bit_length() - 1)) - 1


def period_of(repeat_turn):
    return np.array([t - snapshot_turn(t) if t > 0 else -1 for t in repeat_turn], dtype=np.int64)


def np_periods(cells, rules, turns, at=()):
    """The definition: ({turn: repeat_turn array after that many turns} for the turns in `at` and
    for `turns`, the (n, turns) alive counts, the boards after `turns`)."""
    cells = np.ascontiguousarray(cells, dtype=np.uint8)
    n = cells.shape[0]
    repeat = np.full(n, -1, dtype=np.int64)
    counts = np.zeros((n, turns), dtype=np.int64)
    records = {}
    snap, cur = cells, cells
    for t in range(1, turns + 1):
        cur = np_step_boards(cur, rules)
        counts[:, t - 1] = cur.sum(axis=(1, 2))
        same = (cur == snap).all(axis=(1, 2))
        repeat[(repeat < 0) & same] = t
        if (t + 1) & t == 0:  # t = 2^j - 1: the next window's snapshot
            snap = cur
        if t in at or t == turns:
            records[t] = repeat.copy()
    for a in (counts, cur, *records.values()):
        a.setflags(write=False)
    return records, counts, cur


def soups(n, w, h, seed, density=0.37):
    return (np.random.default_rng(seed).random((n, h, w)) < density).astype(np.uint8)


def cells_of(b):
    return (b.store() != 0).astype(np.uint8)


def check_periods(b, repeat, where=""):
    got_turn, got_period = b.periods()
    assert got_turn.dtype == np.int64 and got_period.dtype == np.int64
    bad = np.nonzero(got_turn != repeat)[0]
    assert bad.size == 0, (where, bad[:8], got_turn[bad[:8]], repeat[bad[:8]])
    assert np.array_equal(got_period, period_of(repeat)), where


BLOCK = ["11", "11"]
BLINKER = ["111"]
GLIDER = [".1.", "..1", "111"]
PENTADECATHLON = ["1111111111"]  # period 15, grows to 16 x 9 around its row
PULSAR = ["..111...111..", ".............", "1....1.1....1", "1....1.1....1", "1....1.1....1", "..111...111..",
          ".............", "..111...111..", "1....1.1....1", "1....1.1....1", "1....1.1....1", ".............",
          "..111...111.."]  # period 3, 15 x 15 at its widest


def board_with(w, h, *placed):
    """An h x w board with patterns at (pattern, y, x)."""
    cells = np.zeros((h, w), dtype=np.uint8)
    for pattern, y, x in placed:
        for dy, line in enumerate(pattern):
            for dx, ch in enumerate(line):
                if ch == "1":
                    cells[(y + dy) % h, (x + dx) % w] = 1
    return cells


# ---------------------------------------------------------------- 1. exact small cases
def test_exact_small_cases(golhip):
    """16 x 16 (four words wide, eight replicas of the row, one wave): an empty board and a block are
    (1, 1), a blinker (3, 2), a glider (127, 64) -- and on the glider board every lane but a few
    matches the snapshot at every turn, so a match that does not wait for all lanes shows here."""
    boards = np.stack([board_with(16, 16), board_with(16, 16, (BLOCK, 7, 7)), board_with(16, 16, (BLINKER, 8, 6)),
                       board_with(16, 16, (GLIDER, 1, 1))])
    want_turn, want_period = np.array([1, 1, 3, 127]), np.array([1, 1, 2, 64])
    ref, _, end = np_periods(boards, LIFE, 130, at=(1, 2, 3, 126, 127))
    assert np.array_equal(ref[130], want_turn) and np.array_equal(period_of(ref[130]), want_period)
    with golhip.Batch(16, 16, 4) as b:
        b.load(boards * 255)
        b.track_period()
        assert np.array_equal(b.periods()[0], [-1] * 4) and np.array_equal(b.periods()[1], [-1] * 4)
        done = 0
        for t in (1, 2, 3, 126, 127, 130):
            b.step(t - done)
            done = t
            check_periods(b, ref[t], t)
        got_turn, got_period = b.periods()
        assert np.array_equal(got_turn, want_turn) and np.array_equal(got_period, want_period)
        assert np.array_equal(cells_of(b), end)


# ---------------------------------------------------------------- 2. agreement across waves and segments
def oscillator_boards(w, h, rows):
    """Blinker (2), pulsar (3) and pentadecathlon (15) at the three rows `rows` (owned by different
    waves): all three (30), blinker + pulsar (6), pulsar + pentadecathlon (15), blinker +
    pentadecathlon (30)."""
    yb, yp, yd = rows
    blinker, pulsar, penta = (BLINKER, yb, 20), (PULSAR, yp, 2), (PENTADECATHLON, yd, 30)
    return np.stack([board_with(w, h, blinker, pulsar, penta), board_with(w, h, blinker, pulsar),
                     board_with(w, h, pulsar, penta), board_with(w, h, blinker, penta)])


@pytest.mark.parametrize("w,h,rows", [(64, 64, (56, 1, 36)), (128, 256, (200, 3, 100))], ids=["64x64", "128x256"])
def test_oscillators_in_different_waves_agree_on_one_turn(golhip, w, h, rows):
    """Each oscillator alone matches its snapshot far more often than the board does: the board
    repeats only when the lanes of every wave match at the same turn."""
    boards = oscillator_boards(w, h, rows)
    ref, _, end = np_periods(boards, LIFE, 70, at=(37, 46, 61))
    assert np.array_equal(period_of(ref[70]), [30, 6, 15, 30]), ref[70]
    assert np.array_equal(ref[70], [61, 13, 30, 61]), ref[70]
    with golhip.Batch(w, h, 4) as b:
        b.load(boards * 255)
        b.track_period()
        done = 0
        for t in (37, 46, 61, 70):
            b.step(t - done)
            done = t
            check_periods(b, ref[t], t)
        assert np.array_equal(cells_of(b), end)


def test_a_lone_glider_on_64x64(golhip):
    boards = np.stack([board_with(64, 64, (GLIDER, 30, 30)), board_with(64, 64, (GLIDER, 61, 62))])
    ref, _, end = np_periods(boards, LIFE, 520, at=(510, 511))
    assert np.array_equal(ref[520], [511, 511]) and np.array_equal(period_of(ref[520]), [256, 256])
    assert np.array_equal(ref[510], [-1, -1])
    with golhip.Batch(64, 64, 2) as b:
        b.load(boards * 255)
        b.track_period()
        b.step(510)
        check_periods(b, ref[510], 510)
        b.step(1)
        check_periods(b, ref[511], 511)
        b.step(9)
        check_periods(b, ref[520], 520)
        assert np.array_equal(cells_of(b), end)


# ---------------------------------------------------------------- 3. every (W, R) shape once
# (width, height): every height of the shape table, every width, each of 4, 8 and 16 torus words
# (16, 64, 128 -> 4; 256 -> 8; 512 -> 16), replicated rows at 16 and 64
SHAPES = [(16, 4), (64, 8), (256, 16), (512, 32), (128, 64), (256, 128), (512, 256), (64, 512), (512, 512)]


def shape_boards(w, h):
    if h >= 64:  # constructed: periods 30, 6, 15
        return oscillator_boards(w, h, (h - 8, 1, h // 2))[:3], 70
    if h == 32:  # blinker + pulsar (6), a blinker, a pulsar
        blinker, pulsar = (BLINKER, 24, 40), (PULSAR, 2, 70)
        return np.stack([board_with(w, h, blinker, pulsar), board_with(w, h, blinker), board_with(w, h, pulsar)]), 40
    # short boards: a blinker, a block and soups
    fixed = np.stack([board_with(w, h, (BLINKER, 1, 5)), board_with(w, h, (BLOCK, 1, 9))])
    return np.concatenate([fixed, soups(14, w, h, 7 * w + h)]), 300


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_every_shape(golhip, w, h):
    boards, turns = shape_boards(w, h)
    ref, counts, end = np_periods(boards, LIFE, turns, at=(turns // 2,))
    assert (ref[turns] > 0).any(), ref[turns]
    with golhip.Batch(w, h, boards.shape[0]) as b:
        b.load(boards * 255)
        b.track_period()
        hist = b.step(turns // 2, history=True)
        assert np.array_equal(hist.astype(np.int64), counts[:, :turns // 2])
        check_periods(b, ref[turns // 2], "half")
        b.step(turns - turns // 2)
        check_periods(b, ref[turns], "end")
        assert np.array_equal(cells_of(b), end)


# ---------------------------------------------------------------- 4. soups
SOUP_TURNS = 2048
SOUP_SEEDS = {16: 1, 32: 2}


@functools.lru_cache(maxsize=None)
def soup_reference(size):
    """64 soups of size x size at density 0.37 from SOUP_SEEDS[size]: (the boards, the repeat turns
    after 256 and 2048 turns, the counts, the boards after 2048 turns)."""
    cells = soups(64, size, size, SOUP_SEEDS[size])
    cells.setflags(write=False)
    ref, counts, end = np_periods(cells, LIFE, SOUP_TURNS, at=(256,))
    return cells, ref, counts, end


@pytest.mark.parametrize("size", [16, 32])
def test_soups(golhip, size):
    cells, ref, _, end = soup_reference(size)
    periods = period_of(ref[SOUP_TURNS])
    distinct = set(int(v) for v in periods if v > 0)
    # the reference alone: three or more periods, one above 2, and a board still without a repeat
    # after 256 turns
    assert len(distinct) >= 3 and max(distinct) > 2, distinct
    assert (ref[256] < 0).any(), ref[256]
    with golhip.Batch(size, size, 64) as b:
        b.load(cells * 255)
        b.track_period()
        b.step(256)
        check_periods(b, ref[256], 256)
        b.step(SOUP_TURNS - 256)
        check_periods(b, ref[SOUP_TURNS], SOUP_TURNS)
        assert np.array_equal(cells_of(b), end)


# ---------------------------------------------------------------- 5. cuts
CUTS = [1, 7, 31, 32, 33, 100, 1, 63, 64, 65, 4, 127, 128, 129, 250, 3, 500]
CUTS.append(SOUP_TURNS - sum(CUTS))


def test_the_records_do_not_depend_on_the_cuts(golhip):
    """The 32 x 32 soups in one call of 2048 turns, in calls of 1, 7, 31, 32, 33, 100, ... turns, and
    the same with history: identical records, equal to the reference's, the history that of a
    handle without tracking."""
    cells, ref, counts, end = soup_reference(32)
    assert sum(CUTS) == SOUP_TURNS and min(CUTS) > 0
    with golhip.Batch(32, 32, 64) as plain:
        plain.load(cells * 255)
        plain_hist = plain.step(SOUP_TURNS, history=True)
    assert np.array_equal(plain_hist.astype(np.int64), counts)
    for cuts in ([SOUP_TURNS], CUTS):
        for history in (False, True):
            with golhip.Batch(32, 32, 64) as b:
                b.load(cells * 255)
                b.track_period()
                done = 0
                for n in cuts:
                    hist = b.step(n, history=history)
                    if history:
                        assert np.array_equal(hist, plain_hist[:, done:done + n]), (len(cuts), done)
                    done += n
                    if done == 256:
                        check_periods(b, ref[256], (len(cuts), history, 256))
                check_periods(b, ref[SOUP_TURNS], (len(cuts), history))
                assert np.array_equal(cells_of(b), end)


CHILD = """
import sys
sys.path.insert(0, {pkg!r})
import numpy as np
import golhip
boards = np.load({inp!r})
with golhip.Batch(32, 32, boards.shape[0]) as b:
    b.load(boards)
    b.track_period()
    hist = b.step({turns}, history=True)
    repeat_turn, period = b.periods()
    np.savez({out!r}, hist=hist, end=b.store(), repeat_turn=repeat_turn, period=period)
"""


def test_history_over_many_short_launches(golhip, tmp_path):
    """A fresh process whose stage is 9472 bytes (GOLHIP_STAGE_BYTES): with 64 boards a history launch
    is at most 37 generations deep, so the 2048 turns are 55 launches of 37 and one of 13, whose
    32-generation mask blocks never line up with the windows."""
    cells, ref, counts, end = soup_reference(32)
    np.save(tmp_path / "in.npy", cells * 255)
    code = CHILD.format(pkg=str(PKG), inp=str(tmp_path / "in.npy"), out=str(tmp_path / "out.npz"), turns=SOUP_TURNS)
    env = dict(os.environ, GOLHIP_STAGE_BYTES=str(64 * 4 * 37))
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, "-c", code], env=env, check=True, timeout=120)
    small = np.load(tmp_path / "out.npz")
    assert np.array_equal(small["hist"].astype(np.int64), counts)
    assert np.array_equal(small["repeat_turn"], ref[SOUP_TURNS])
    assert np.array_equal(small["period"], period_of(ref[SOUP_TURNS]))
    assert np.array_equal((small["end"] != 0).astype(np.uint8), end)


# ---------------------------------------------------------------- 6. rules
@pytest.mark.parametrize("rule,form,density", [(HIGHLIFE, 1, 0.37), (TABLE_RULE, 2, 0.03)], ids=["highlife", "table"])
def test_uniform_rules(golhip, rule, form, density):
    """32 soups of 32 x 32 (the table rule keeps lone cells alive: sparse soups freeze, dense ones burn
    on) with an empty board first; the reference shows periods 1 and 2 and boards without a repeat."""
    cells = soups(32, 32, 32, 11, density)
    cells[0] = 0
    ref, counts, end = np_periods(cells, rule, 600, at=(100,))
    assert set(period_of(ref[600])) >= {-1, 1, 2}, ref[600]
    with golhip.Batch(32, 32, 32, rule=rule) as b:
        assert b.kernel_form == form
        b.load(cells * 255)
        b.track_period()
        assert b.kernel_form == form  # the form names the rule, not the tracking
        hist = b.step(100, history=True)
        assert np.array_equal(hist.astype(np.int64), counts[:, :100])
        check_periods(b, ref[100], 100)
        b.step(500)
        check_periods(b, ref[600], 600)
        assert np.array_equal(cells_of(b), end)


def test_one_rule_per_board(golhip):
    """B3/S23, a catalogue rule, the table rule and a strobing B0 rule side by side (form 3); the
    first four boards are empty: (1, 1) three times and the strobe's (3, 2)."""
    rules = [LIFE, HIGHLIFE, TABLE_RULE, STROBE] * 8
    cells = soups(32, 32, 32, 13)
    cells[:4] = 0
    ref, counts, end = np_periods(cells, rules, 600, at=(3, 100))
    assert np.array_equal(ref[3][:4], [1, 1, 1, 3]) and np.array_equal(period_of(ref[3])[:4], [1, 1, 1, 2])
    assert len(set(period_of(ref[600]))) >= 3
    with golhip.Batch(32, 32, 32, rules=rules) as b:
        assert b.kernel_form == 3
        b.load(cells * 255)
        b.track_period()
        b.step(3)
        check_periods(b, ref[3], 3)
        hist = b.step(97, history=True)
        assert np.array_equal(hist.astype(np.int64), counts[:, 3:100])
        check_periods(b, ref[100], 100)
        b.step(500)
        check_periods(b, ref[600], 600)
        assert np.array_equal(cells_of(b), end)


# ---------------------------------------------------------------- 7. state rules
def test_state_rules(golhip):
    cells = soups(3, 64, 64, 3)
    cells[0] = board_with(64, 64, (BLINKER, 5, 5))
    with golhip.Batch(64, 64, 3) as b:
        b.load(cells * 255)
        with pytest.raises(golhip.GolHipError) as ei:  # nothing to ask for yet
            b.periods()
        assert ei.value.code == golhip.ERR_STATE
        b.step(1)
        with pytest.raises(golhip.GolHipError) as ei:  # board(0) is the first snapshot
            b.track_period()
        assert ei.value.code == golhip.ERR_STATE and b.turn == 1
        with pytest.raises(golhip.GolHipError) as ei:
            b.periods()
        assert ei.value.code == golhip.ERR_STATE
        # one tracker at a time
        b.load(cells * 255)
        b.track_settle()
        with pytest.raises(golhip.GolHipError) as ei:
            b.track_period()
        assert ei.value.code == golhip.ERR_STATE and "settle" in str(ei.value) and "period" in str(ei.value)
        assert b.settled().shape == (3,)
        b.track_settle(False)
        b.track_period()
        with pytest.raises(golhip.GolHipError) as ei:
            b.track_settle()
        assert ei.value.code == golhip.ERR_STATE and "settle" in str(ei.value) and "period" in str(ei.value)
        # either output may be left out
        lib = golhip.load_library()
        b.step(3)
        only = np.zeros(3, dtype=np.int64)
        assert lib.golhip_batch_periods(b._h, None, only.ctypes.data) == golhip.OK and only[0] == 2
        assert lib.golhip_batch_periods(b._h, only.ctypes.data, None) == golhip.OK and only[0] == 3
        assert lib.golhip_batch_periods(b._h, None, None) == golhip.OK
        # a load resets the records
        assert b.periods()[0][0] == 3
        b.load(cells * 255)
        assert b.turn == 0
        assert np.array_equal(b.periods()[0], [-1] * 3) and np.array_equal(b.periods()[1], [-1] * 3)
        # the record is the record of one rule
        b.set_rule(TABLE_RULE)  # at turn 0: fine
        b.step(2)
        before = cells_of(b)
        for change in (lambda: b.set_rule("B3/S23"), lambda: b.set_rule(HIGHLIFE),
                       lambda: b.set_rules([LIFE, HIGHLIFE, TABLE_RULE])):
            with pytest.raises(golhip.GolHipError) as ei:
                change()
            assert ei.value.code == golhip.ERR_STATE
        assert b.rule_masks == TABLE_RULE and b.kernel_form == 2 and b.turn == 2
        assert np.array_equal(cells_of(b), before)
        b.set_rule(TABLE_RULE)  # the rule it has: no change
        ref, _, end = np_periods(cells, TABLE_RULE, 9)
        b.step(7)
        check_periods(b, ref[9], "table rule")
        assert np.array_equal(cells_of(b), end)


def test_tracking_off_changes_nothing(golhip):
    """A handle that enabled tracking and switched it off again runs what a handle that never
    enabled it runs: the same boards and history."""
    cells = soups(5, 128, 64, 19)
    runs = []
    for touched in (False, True):
        with golhip.Batch(128, 64, 5) as b:
            b.load(cells * 255)
            if touched:
                b.track_period()
                b.track_period(False)
                with pytest.raises(golhip.GolHipError) as ei:
                    b.periods()
                assert ei.value.code == golhip.ERR_STATE
            runs.append((b.step(45, history=True), b.store()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    _, counts, end = np_periods(cells, LIFE, 45)
    assert np.array_equal(runs[0][0].astype(np.int64), counts)
    assert np.array_equal((runs[0][1] != 0).astype(np.uint8), end)
