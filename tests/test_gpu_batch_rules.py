"""Life-like rules on golhip.Batch (golhip_batch_set_rule / _set_rules, the kernel gol_batch_rule of
csrc/batch_rule.hpp): one rule for all boards -- constant-folded for the catalogue, the table form
for every other rule -- or one rule per board (always the table form), through every board shape,
the history, several launches per call, settling and more boards than are resident.

The oracle is B3/S23 only, so the reference is the numpy stepper np_step of tests/test_gpu_rules.py
(and np_step_boards below: the same eight rolls over a stack of boards, each under its own rule);
everything is bit-exact."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from test_gpu_rules import ANTILIFE, CATALOGUE, HIGHLIFE, TABLE_RULE, np_step, random_cells, truth_rules

pytestmark = pytest.mark.gpu

LIFE = (0x008, 0x00C)
MAZE = (0x008, 0x03E)        # B3/S12345
REPLICATOR = (0x0AA, 0x0AA)  # B1357/S1357, constant-folded


def np_step_boards(cells, rules):
    """One generation of an (n, h, w) stack of 0/1 tori, board i under rules[i] = (birth, survive)
    (a single pair: every board under it)."""
    rules = np.asarray(rules, dtype=np.int64).reshape(-1, 2)
    birth, survive = rules[:, 0].reshape(-1, 1, 1), rules[:, 1].reshape(-1, 1, 1)
    c = cells.astype(np.int64)
    n = sum(np.roll(np.roll(c, dy, 1), dx, 2) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    return np.where(cells == 1, (survive >> n) & 1, (birth >> n) & 1).astype(np.uint8)


def np_run_boards(cells, rules, turns):
    """(the boards after `turns` generations, the (n, turns) alive counts of generations 1..turns)."""
    counts = np.zeros((cells.shape[0], turns), dtype=np.int64)
    for t in range(turns):
        cells = np_step_boards(cells, rules)
        counts[:, t] = cells.sum(axis=(1, 2))
    return cells, counts


def soups(n, w, h, seed, density=0.37):
    return (np.random.default_rng(seed).random((n, h, w)) < density).astype(np.uint8)


def cells_of(b):
    return (b.store() != 0).astype(np.uint8)


# ---------------------------------------------------------------- 1. truth tables, one rule per board
def test_truth_tables_one_rule_per_board(golhip):
    """72 rules (the catalogue, B3/S23, the empty and the full rule, AntiLife, 64 seeded random mask
    pairs) on 72 copies of one dense board that holds every (state, neighbour count) pair: one
    generation, then four more (a group of 4 and a remainder of 1, in two launches)."""
    rules = truth_rules()
    assert len(rules) == 72
    cells = random_cells(128, 64, 1)
    c = cells.astype(np.int64)
    n = sum(np.roll(np.roll(c, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    for state in (0, 1):
        for k in range(9):
            assert np.count_nonzero((cells == state) & (n == k)) >= 10, (state, k)
    with golhip.Batch(128, 64, 72) as b:
        assert b.kernel_form == 0 and b.rule == "B3/S23"
        b.load(np.tile(cells * 255, (72, 1, 1)))
        b.set_rules(rules)
        assert b.kernel_form == 3
        assert np.array_equal(b.rules, np.array(rules, dtype=np.uint32))
        hist = b.step(1, history=True)
        got = cells_of(b)
        gen1 = []
        for i, rule in enumerate(rules):
            exp = np_step(cells, rule)
            gen1.append(exp)
            assert np.array_equal(got[i], exp), (i, golhip.rule_string(*rule))
            assert int(hist[i, 0]) == int(exp.sum()), (i, golhip.rule_string(*rule))
        b.step(4)
        assert b.turn == 5
        got = cells_of(b)
        for i, rule in enumerate(rules):
            exp = gen1[i]
            for _ in range(4):
                exp = np_step(exp, rule)
            assert np.array_equal(got[i], exp), (i, golhip.rule_string(*rule))
        assert np.array_equal(b.rules, np.array(rules, dtype=np.uint32))


# ---------------------------------------------------------------- 2. every shape, uniform rules
HEIGHTS = [4, 8, 16, 32, 64, 128, 256, 512]
SHAPES = [((128, 256, 512)[i % 3], h) for i, h in enumerate(HEIGHTS) if h != 16]
SHAPES += [(w, 16) for w in (128, 256, 512, 16, 64)]  # 16 / 64: replicated rows, a partial count mask
UNIFORM = [(HIGHLIFE, 1), (TABLE_RULE, 2), (ANTILIFE, 2)]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("rule,form", UNIFORM, ids=["highlife", "table", "antilife"])
def test_every_shape_under_a_uniform_rule(golhip, w, h, rule, form):
    """5 boards at density 0.37, 11 turns with history (two groups of 4 and a remainder of 3): the
    boards, every history count and alive_counts()."""
    cells = soups(5, w, h, 31 * w + h)
    exp, exp_counts = np_run_boards(cells, rule, 11)
    with golhip.Batch(w, h, 5, rule=rule) as b:
        assert b.kernel_form == form and b.rule_masks == rule
        b.load(cells * 255)
        hist = b.step(11, history=True)
        assert np.array_equal(hist.astype(np.int64), exp_counts)
        assert np.array_equal(cells_of(b), exp)
        assert np.array_equal(b.alive_counts().astype(np.int64), exp_counts[:, -1])


# ---------------------------------------------------------------- 3. the catalogue
@pytest.mark.parametrize("rule", CATALOGUE, ids=["highlife", "daynight", "seeds", "replicator"])
def test_catalogue_rules_run_constant_folded(golhip, rule):
    cells = soups(3, 64, 64, 5, 0.5)
    exp, exp_counts = np_run_boards(cells, rule, 9)
    with golhip.Batch(64, 64, 3) as b:
        b.set_rule(golhip.rule_string(*rule))
        assert b.kernel_form == 1 and b.rule_masks == rule
        b.load(cells * 255)
        hist = b.step(9, history=True)
        assert np.array_equal(hist.astype(np.int64), exp_counts)
        assert np.array_equal(cells_of(b), exp)


# ---------------------------------------------------------------- 4. several launches per call
CHILD = """
import sys
sys.path.insert(0, {pkg!r})
import numpy as np
import golhip
boards = np.load({inp!r})
with golhip.Batch(64, 32, boards.shape[0], rule="B36/S23") as b:
    b.load(boards)
    hist = b.step(37, history=True)
    np.savez({out!r}, hist=hist, end=b.store(), form=b.kernel_form)
"""


def test_history_over_several_launches(golhip, tmp_path):
    """A fresh process whose stage is 192 bytes (GOLHIP_STAGE_BYTES): with 6 boards a history launch
    is at most 8 generations deep, so 37 turns of HighLife are launches of 8, 8, 8, 8 and 5."""
    cells = soups(6, 64, 32, 17)
    exp, exp_counts = np_run_boards(cells, HIGHLIFE, 37)
    np.save(tmp_path / "in.npy", cells * 255)
    code = CHILD.format(pkg=str(PKG), inp=str(tmp_path / "in.npy"), out=str(tmp_path / "out.npz"))
    env = dict(os.environ, GOLHIP_STAGE_BYTES="192")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, "-c", code], env=env, check=True, timeout=120)
    small = np.load(tmp_path / "out.npz")
    assert int(small["form"]) == 1
    assert np.array_equal(small["hist"].astype(np.int64), exp_counts)
    assert np.array_equal((small["end"] != 0).astype(np.uint8), exp)


# ---------------------------------------------------------------- 5. settling
SETTLE_BOARDS, SETTLE_TURNS = 16, 600


@functools.lru_cache(maxsize=None)
def settle_reference(rule):
    """16 boards of 32 x 32, board i from default_rng(1000 + i) at density 0.37: (the boards, per
    board the smallest t >= 2 with gen(t) == gen(t - 2) within 600 turns or -1, the counts, the
    boards after 600 turns), by the numpy stepper."""
    cells = np.stack([(np.random.default_rng(1000 + i).random((32, 32)) < 0.37).astype(np.uint8)
                      for i in range(SETTLE_BOARDS)])
    settled = np.full(SETTLE_BOARDS, -1, dtype=np.int64)
    counts = np.zeros((SETTLE_BOARDS, SETTLE_TURNS), dtype=np.int64)
    before2, before, cur = None, None, cells
    for t in range(1, SETTLE_TURNS + 1):
        before2, before, cur = before, cur, np_step_boards(cur, rule)
        counts[:, t - 1] = cur.sum(axis=(1, 2))
        if before2 is not None:
            same = (cur == before2).all(axis=(1, 2))
            settled[(settled < 0) & same] = t
    for a in (cells, settled, counts, cur):
        a.setflags(write=False)
    return cells, settled, counts, cur


@pytest.mark.parametrize("rule", [MAZE, REPLICATOR, HIGHLIFE, ANTILIFE],
                         ids=["maze", "replicator", "highlife", "antilife"])
def test_boards_settle_when_the_reference_says(golhip, rule):
    """settled() after 600 turns, run in one call and cut as 250 + 350, with and without history,
    equals the reference's settle turns under every rule (AntiLife: the strobing period-2 case)."""
    cells, exp, exp_counts, end = settle_reference(rule)
    if rule in (MAZE, REPLICATOR):
        assert (exp >= 2).all()
    else:  # both branches stay covered
        assert np.count_nonzero(exp >= 2) >= 8 and np.count_nonzero(exp < 0) >= 1, exp
    for cuts in ((600,), (250, 350)):
        for history in (False, True):
            with golhip.Batch(32, 32, SETTLE_BOARDS, rule=rule) as b:
                b.load(cells * 255)
                b.track_settle()
                done = 0
                for n in cuts:
                    hist = b.step(n, history=history)
                    if history:
                        assert np.array_equal(hist.astype(np.int64), exp_counts[:, done:done + n]), (cuts, done)
                    done += n
                    got = b.settled()
                    assert np.array_equal(got, np.where((exp >= 0) & (exp <= done), exp, -1)), (cuts, history, got, exp)
                assert np.array_equal(cells_of(b), end), (cuts, history)


# ---------------------------------------------------------------- 6. more boards than are resident
def test_more_boards_than_are_resident_one_rule_each(golhip):
    """4099 boards of 16 x 16, each under its own seeded random rule, 6 turns."""
    n = 4099
    rules = np.random.default_rng(23).integers(0, 512, (n, 2)).astype(np.uint32)
    cells = soups(n, 16, 16, 29, 0.5)
    exp, exp_counts = np_run_boards(cells, rules, 6)
    with golhip.Batch(16, 16, n, rules=rules) as b:
        assert b.kernel_form == 3
        b.load(cells * 255)
        hist = b.step(6, history=True)
        got = cells_of(b)
        assert np.array_equal(b.rules, rules)
    bad = np.nonzero((got != exp).any(axis=(1, 2)))[0]
    assert bad.size == 0, bad[:10]
    assert np.array_equal(hist.astype(np.int64), exp_counts)


# ---------------------------------------------------------------- 7. B3/S23 three ways
def test_life_three_ways(golhip, oracle):
    """The same 64 x 64 soups for 20 turns with history by gol_batch (default, and B3/S23 set
    explicitly: form 0) and by the table kernel with per-board rules that are all B3/S23 (form 3):
    identical, and equal to the oracle."""
    boards = soups(4, 64, 64, 41, 0.5) * 255
    runs = []
    for how in ("default", "explicit", "per board"):
        with golhip.Batch(64, 64, 4) as b:
            if how == "explicit":
                b.set_rule("B3/S23")
            elif how == "per board":
                b.set_rules([LIFE] * 4)
            assert b.kernel_form == (3 if how == "per board" else 0), how
            b.load(boards)
            hist = b.step(20, history=True)
            runs.append((hist, b.store()))
    for hist, end in runs[1:]:
        assert np.array_equal(hist, runs[0][0]) and np.array_equal(end, runs[0][1])
    for i in range(4):
        ref, counts = oracle.packed_run(boards[i], 20, threads=1)
        assert np.array_equal(runs[0][1][i], ref), i
        assert np.array_equal(runs[0][0][i].astype(np.int64), counts), i


# ---------------------------------------------------------------- 8. contract
def test_contract(golhip):
    cells = soups(3, 64, 64, 3)
    with golhip.Batch(64, 64, 3) as b:
        b.load(cells * 255)
        b.step(2)
        after2 = np_run_boards(cells, LIFE, 2)[0]
        b.set_rule("B36/S23")  # a rule change keeps the boards and the turn
        assert b.turn == 2 and np.array_equal(cells_of(b), after2)
        assert b.rule == "B36/S23" and b.rule_masks == HIGHLIFE and b.kernel_form == 1
        b.step(3)
        after5 = np_run_boards(after2, HIGHLIFE, 3)[0]
        assert b.turn == 5 and np.array_equal(cells_of(b), after5)
        b.load(cells * 255)  # load keeps the rule
        assert b.turn == 0 and b.rule_masks == HIGHLIFE and b.kernel_form == 1
        per_board = [HIGHLIFE, TABLE_RULE, "B3/S23"]
        b.set_rules(per_board)
        masks = np.array([HIGHLIFE, TABLE_RULE, LIFE], dtype=np.uint32)
        assert b.kernel_form == 3 and np.array_equal(b.rules, masks)
        with pytest.raises(golhip.GolHipError) as ei:  # no single rule to report
            b.rule_masks
        assert ei.value.code == golhip.ERR_STATE
        b.step(4)
        assert np.array_equal(cells_of(b), np_run_boards(cells, masks, 4)[0])
        b.load(cells * 255)
        assert b.kernel_form == 3 and np.array_equal(b.rules, masks)
        b.set_rules(None)  # back to the uniform rule
        assert b.kernel_form == 1 and b.rule_masks == HIGHLIFE
        assert np.array_equal(b.rules, np.array([HIGHLIFE] * 3, dtype=np.uint32))
        # invalid masks: refused, the rule unchanged
        with pytest.raises(golhip.GolHipError) as ei:
            b.set_rule((0x200, 0))
        assert ei.value.code == golhip.ERR_ARG and "0x200" in str(ei.value)
        lib = golhip.load_library()
        birth = np.array([8, 8, 0x200], dtype=np.uint32)
        survive = np.array([12, 12, 12], dtype=np.uint32)
        assert lib.golhip_batch_set_rules(b._h, birth.ctypes.data, survive.ctypes.data) == golhip.ERR_ARG
        msg = lib.golhip_batch_last_error(b._h).decode()
        assert "2" in msg and "0x200" in msg, msg
        assert lib.golhip_batch_set_rules(b._h, birth.ctypes.data, None) == golhip.ERR_ARG  # one array only
        assert b.kernel_form == 1 and b.rule_masks == HIGHLIFE
        b.step(5)
        assert np.array_equal(cells_of(b), np_run_boards(cells, HIGHLIFE, 5)[0])
        # settle tracking: the record means something under one rule only
        b.load(cells * 255)
        b.track_settle()
        b.set_rule(TABLE_RULE)  # at turn 0: fine
        b.step(1)
        for change in (lambda: b.set_rule("B3/S23"), lambda: b.set_rule(HIGHLIFE), lambda: b.set_rules(per_board)):
            with pytest.raises(golhip.GolHipError) as ei:
                change()
            assert ei.value.code == golhip.ERR_STATE
        assert b.rule_masks == TABLE_RULE and b.kernel_form == 2 and b.turn == 1
        b.set_rule(TABLE_RULE)  # the rule it has: no change
        b.load(cells * 255)  # a fresh load: turn 0 again
        b.set_rule("B3/S23")
        assert b.kernel_form == 0
        b.set_rules(per_board)
        assert b.kernel_form == 3
        b.step(3)
        assert np.array_equal(cells_of(b), np_run_boards(cells, masks, 3)[0])
        assert b.settled().shape == (3,)
