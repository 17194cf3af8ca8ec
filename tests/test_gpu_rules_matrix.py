"""gol_rule<K, COUNT, LD, Rule> (csrc/golhip_rule.hpp) at every depth, functor and launch path it
ships: 4 depths (8 / 4 / 2 / 1) x COUNT x LD x 5 functors (RuleConst for HighLife, Day & Night, Seeds
and Replicator; RuleTable for every other rule), on single strips down to one row, on strips that
take the K = 8 interior + boundary split, in rank mode as the RCCL ring of one, through rule changes
between functor kinds and through a checkpoint.  tests/test_gpu_rules.py holds the first layer
(truth tables, geometry, the CLI); two real ranks under a rule are in tests/test_gpu_rank_host.py.

The reference is test_gpu_rules' numpy stepper (eight rolls summed in int64, then a mask lookup),
cached; tests/test_rules_cpu.py checks it against the oracle at B3/S23 down to one row.  Everything
is bit-exact: boards, every per-turn count, flips lists.  Every reference passes a liveness guard
before the GPU result is looked at (alive(): the last generation is neither empty nor full and at
least 1 % of the cells changed in it), since a board that died proves nothing about a rule.
Boards start from density 0.5, seed w * 31 + h.  Seeds (B2/S) dies on boards 1 and 3 rows high (at
h = 1 a cell's neighbour count is 3 l + 3 r, never 2), so it runs at h = 2, 5, 7 only.
"""
import functools

import numpy as np
import pytest

from test_gpu_rules import (ANTILIFE, CATALOGUE, HIGHLIFE, TABLE_RULE, cells_of, flips_of, np_run, random_cells,
                            reference)

pytestmark = pytest.mark.gpu

LIFE = (0x008, 0x00C)
DAYNIGHT, SEEDS, REPLICATOR = CATALOGUE[1], CATALOGUE[2], CATALOGUE[3]
NAMES = {HIGHLIFE: "highlife", DAYNIGHT: "daynight", SEEDS: "seeds", REPLICATOR: "replicator",
         TABLE_RULE: "b38s0236", ANTILIFE: "antilife", LIFE: "life"}


def kind_of(rule):
    return ("rule", 1 if rule in CATALOGUE else 0)


def alive(gens, upto=None):
    """The liveness guard, from the reference alone: generation `upto` (default: the last) is
    neither empty nor full, and at least 1 % of the cells differ from the generation before."""
    t = len(gens) - 1 if upto is None else upto
    cur, prev = gens[t], gens[t - 1]
    n = int(cur.sum())
    assert 0 < n < cur.size, (t, n)
    assert 100 * np.count_nonzero(cur != prev) >= cur.size, (t, np.count_nonzero(cur != prev), cur.size)
    return True


def ref_of(w, h, rule, turns, guard_at=()):
    """The cached reference of the board seeded w * 31 + h, guarded at its last generation and at
    every generation of guard_at (the ends of the legs that stop earlier)."""
    gens, counts = reference(w, h, w * 31 + h, rule, turns)
    for t in (*guard_at, turns):
        assert alive(gens, t)
    return gens, counts


def i64(a):
    return np.asarray(a).astype(np.int64)


def life_by_complement(oracle, cells, turns):
    """(board, counts) of AntiLife after `turns` from `cells`, by the project's oracle: AntiLife of
    a board is the complement of Life of its complement."""
    ref, life_counts = oracle.packed_run((1 - cells) * 255, turns)
    return 1 - (ref != 0).astype(np.uint8), cells.size - i64(life_counts)


# ---------------------------------------------------------------- 1. every functor x depth x COUNT x LD
SIX = [HIGHLIFE, DAYNIGHT, SEEDS, REPLICATOR, TABLE_RULE, ANTILIFE]
FULL_W, FULL_H = 3968, 24  # wd = 124: two exactly-full 62-word chunks; three 8-row bands


@pytest.mark.parametrize("d", [8, 4, 2, 1])
@pytest.mark.parametrize("rule", SIX, ids=[NAMES[r] for r in SIX])
def test_every_functor_depth_count_and_flips_form(golhip, rule, d):
    """3 d turns in launches exactly d deep (set_k(d)) on 3968 x 24 -- lane 63 of both chunks has
    colraw == wd, the upper bound of the count window, and wraps to column 0 -- in four legs:
    <d, true, false, F>, <d, false, false, F>, tracking with counts <d, true, true, F> (the last
    launch; the two before it <d, true, false, F>) and tracking without <d, false, true, F>, F the
    rule's functor: RuleConst<B, S> for the catalogue, RuleTable for B38/S0236 and AntiLife."""
    turns = 3 * d
    gens, exp_counts = ref_of(FULL_W, FULL_H, rule, turns)
    exp_flips = flips_of(gens[turns - 1], gens[turns])
    with golhip.Engine(FULL_W, FULL_H, k=8, rule=rule) as e:
        assert e.info.torus_width == FULL_W
        e.set_k(d)
        assert e.launch_kind(d, counts=True) == kind_of(rule) == e.launch_kind(d)
        for track in (False, True):
            e.track_flips(track)
            e.load(gens[0] * 255)
            counts = e.step(turns, counts=True)
            assert np.array_equal(i64(counts), exp_counts), (track, counts, exp_counts)
            if track:
                assert np.array_equal(e.flips(), exp_flips)
            assert np.array_equal(cells_of(e), gens[turns]), track
            e.load(gens[0] * 255)
            e.step(turns)
            if track:
                assert np.array_equal(e.flips(), exp_flips)
            assert np.array_equal(cells_of(e), gens[turns]), track
        assert e.turn == turns


@pytest.mark.parametrize("rule", SIX, ids=[NAMES[r] for r in SIX])
def test_every_functor_through_the_depth_ladder(golhip, oracle, rule):
    """One 23-turn call at k = 8 with counts: <8, true, false, F> twice, then <4 | 2 | 1, true,
    false, F> on the board the level before left, for each of the five functors (and AntiLife, the
    second table rule, also against the oracle through the complement)."""
    gens, exp_counts = ref_of(FULL_W, FULL_H, rule, 23)
    with golhip.Engine(FULL_W, FULL_H, k=8, rule=rule) as e:
        assert e.launch_kind(8, counts=True) == kind_of(rule)
        e.load(gens[0] * 255)
        counts = e.step(23, counts=True)
        got = cells_of(e)
    assert np.array_equal(i64(counts), exp_counts), (counts, exp_counts)
    assert np.array_equal(got, gens[23])
    if rule == ANTILIFE:
        board, life_counts = life_by_complement(oracle, gens[0], 23)
        assert np.array_equal(got, board) and np.array_equal(i64(counts), life_counts)


# ---------------------------------------------------------------- 2. tiny heights
TINY_RULES = [HIGHLIFE, REPLICATOR, TABLE_RULE, ANTILIFE]


@pytest.mark.parametrize("h", [1, 2, 3, 5, 7, 9, 15])
@pytest.mark.parametrize("w", [128, 48])
def test_boards_shorter_than_the_pipeline(golhip, w, h):
    """Boards of 1 .. 15 rows, one strip: RowStream(p, ya - K) wraps the torus several times inside
    the 2 K-row pipeline fill, the P-block overrun reloads wrapped rows, at h = 1, 2, 3 the three
    neighbour rows coincide.  w = 128: wd = 4, one chunk that wraps inside the wave; w = 48: the
    replicated torus, L = 384.  At set_k(8) 24 turns are <8, COUNT, false, F> x 3, at set_k(1)
    <1, COUNT, false, F> x 24, COUNT both ways; then 9 ring turns <1, true, true, F>, every turn's
    flips.  F: RuleConst of HighLife and Replicator (and of Seeds at h = 2, 5, 7), RuleTable of
    B38/S0236 and AntiLife."""
    rules = TINY_RULES + ([SEEDS] if h in (2, 5, 7) else [])
    with golhip.Engine(w, h, k=8) as e:
        for rule in rules:
            gens, exp_counts = ref_of(w, h, rule, 33, guard_at=(24,))
            e.set_rule(rule)
            for d in (8, 1):
                tag = (NAMES[rule], d)
                e.set_k(d)
                assert e.launch_kind(d, counts=True) == kind_of(rule), tag
                e.load(gens[0] * 255)
                counts = e.step(24, counts=True)
                assert np.array_equal(i64(counts), exp_counts[:24]), (tag, counts, exp_counts[:24])
                assert np.array_equal(cells_of(e), gens[24]), tag
                e.load(gens[0] * 255)
                e.step(24)
                assert np.array_equal(cells_of(e), gens[24]), tag
                per_turn, ring_counts = e.step_flips(9, counts=True)
                assert np.array_equal(i64(ring_counts), exp_counts[24:33]), tag
                for t in range(9):
                    assert np.array_equal(per_turn[t], flips_of(gens[24 + t], gens[25 + t])), (tag, t)
                assert np.array_equal(cells_of(e), gens[33]), tag


# ---------------------------------------------------------------- 3. strips that take the K = 8 split
STRIP_RULES = [HIGHLIFE, DAYNIGHT, TABLE_RULE, ANTILIFE]


def run_strip_legs(e, gens):
    """27 turns with counts; 16 turns with tracking; 5 ring turns: what each left behind."""
    out = {}
    e.load(gens[0] * 255)
    out["counts27"] = i64(e.step(27, counts=True))
    out["board27"] = cells_of(e)
    e.load(gens[0] * 255)
    e.track_flips(True)
    e.step(16)
    out["flips16"] = e.flips().copy()
    out["board16"] = cells_of(e)
    e.track_flips(False)
    e.load(gens[0] * 255)
    per_turn, ring_counts = e.step_flips(5, counts=True)
    out["ring_counts"] = i64(ring_counts)
    out["ring_flips"] = [x.copy() for x in per_turn]
    out["board5"] = cells_of(e)
    return out


@pytest.mark.parametrize("h", [72, 76, 100])
@pytest.mark.parametrize("w", [2048, 48])
@pytest.mark.parametrize("rule", STRIP_RULES, ids=[NAMES[r] for r in STRIP_RULES])
def test_strips_take_the_interior_and_boundary_launches(golhip, oracle, rule, w, h):
    """Three strips of >= 3 K = 24 rows at k = 8 in halo mode: every 8-deep launch is the halo-free
    interior (rows [8, rows - 8); at h = 72 exactly [8, 16)) beside the two-range boundary launch
    (rows [0, 8) and [rows - 8, rows)) on the edge stream, rows outside a strip clamped -- under
    AntiLife (B0) what is computed from them is alive, not dead.  27 turns with counts:
    <8, true, false, F> x 3, then <2, ..> and <1, ..>; 16 turns with tracking: <8, false, false, F>
    then <8, false, true, F>; 5 ring turns: <1, true, true, F>.  F: RuleConst of HighLife and Day &
    Night, RuleTable of B38/S0236 and AntiLife.  Against the reference and a single strip."""
    bounds = [golhip.strip_bounds(h, 3, r) for r in range(3)]
    assert [b[0] for b in bounds] == [0, bounds[0][1], bounds[0][1] + bounds[1][1]]
    assert sum(b[1] for b in bounds) == h and all(b[1] >= 24 for b in bounds)
    if h == 72:
        assert [b[1] for b in bounds] == [24, 24, 24]
    if h == 76:
        assert [b[1] for b in bounds] == [25, 25, 26]
    gens, exp_counts = ref_of(w, h, rule, 27, guard_at=(5, 16))
    with golhip.Engine(w, h, ngpus=1, k=8, strips=3, rule=rule) as e:
        assert e.info.world_size == 3 and e.info.halo_rows >= 8
        assert e.launch_kind(8, counts=True) == kind_of(rule)
        got = run_strip_legs(e, gens)
    with golhip.Engine(w, h, k=8, rule=rule) as e:
        single = run_strip_legs(e, gens)
    for name, res in (("strips", got), ("single", single)):
        assert np.array_equal(res["counts27"], exp_counts), (name, res["counts27"], exp_counts)
        assert np.array_equal(res["board27"], gens[27]), name
        assert np.array_equal(res["flips16"], flips_of(gens[15], gens[16])), name
        assert np.array_equal(res["board16"], gens[16]), name
        assert np.array_equal(res["ring_counts"], exp_counts[:5]), name
        for t in range(5):
            assert np.array_equal(res["ring_flips"][t], flips_of(gens[t], gens[t + 1])), (name, t)
        assert np.array_equal(res["board5"], gens[5]), name
    if rule == ANTILIFE:
        board, life_counts = life_by_complement(oracle, gens[0], 27)
        assert np.array_equal(got["board27"], board) and np.array_equal(got["counts27"], life_counts)


# ---------------------------------------------------------------- 4. rank mode, the RCCL ring of one
RANK_RULES = [HIGHLIFE, TABLE_RULE, ANTILIFE]


@pytest.mark.parametrize("rule", RANK_RULES, ids=[NAMES[r] for r in RANK_RULES])
def test_rank_mode_ring_of_one_under_a_rule(golhip, oracle, monkeypatch, rule):
    """Rank mode over RCCL (GOLHIP_RING_SELF=1: one halo'd strip of 77 rows, 640 wide, k = 8): the
    interior launch enqueued before the exchange (interior_first), the boundary bands behind the
    ncclSend / ncclRecv halos, the counts through ncclAllReduce.  27 turns with counts
    (<8, true, false, F> x 3, <2, ..>, <1, ..>, each an interior and a boundary launch), then 9
    without (<8, false, false, F>, <1, ..>).  F: RuleConst<B36/S23>, RuleTable (B38/S0236, AntiLife)."""
    monkeypatch.setenv("GOLHIP_RING_SELF", "1")
    w, h = 640, 77
    gens, exp_counts = ref_of(w, h, rule, 36, guard_at=(27,))
    with golhip.Engine(w, h, k=8, rank=0, world_size=1, device=0, rule=rule) as e:
        assert e.info.halo_rows == 8 and e.info.world_size == 1
        assert e.launch_kind(8, counts=True) == kind_of(rule)
        e.load(gens[0] * 255)
        counts = e.step(27, counts=True)
        mid = cells_of(e)
        n_mid = e.alive_count()
        e.step(9)
        got = cells_of(e)
        n = e.alive_count()
        assert e.turn == 36
    assert np.array_equal(i64(counts), exp_counts[:27]), (counts, exp_counts[:27])
    assert np.array_equal(mid, gens[27]) and n_mid == int(exp_counts[26])
    assert np.array_equal(got, gens[36]) and n == int(exp_counts[35])
    if rule == ANTILIFE:
        board, life_counts = life_by_complement(oracle, gens[0], 36)
        assert np.array_equal(got, board) and np.array_equal(i64(counts), life_counts[:27])


# ---------------------------------------------------------------- 6. rule changes and the checkpoint
SWITCH_W, SWITCH_H = 2048, 40
SWITCHES = [HIGHLIFE, TABLE_RULE, DAYNIGHT, LIFE]


@functools.lru_cache(maxsize=None)
def switch_reference():
    """[(generations, counts)] of 24 turns under each rule of SWITCHES in turn, each from where the
    rule before left the board."""
    cells = random_cells(SWITCH_W, SWITCH_H, SWITCH_W * 31 + SWITCH_H)
    legs = []
    for rule in SWITCHES:
        gens, counts = np_run(cells, rule, 24)
        legs.append((gens, counts))
        cells = gens[-1]
    return legs


def test_rule_changes_between_functor_kinds_at_depth(golhip):
    """One handle, k = 8, counts on: HighLife (RuleConst), B38/S0236 (RuleTable), Day & Night
    (RuleConst) and B3/S23 (the production kernels) for 24 turns each -- <8, true, false, F> x 3 per
    rule, the occupancy cache of the rule before dropped and a new band plan made at each switch."""
    legs = switch_reference()
    with golhip.Engine(SWITCH_W, SWITCH_H, k=8) as fresh:
        fresh_kinds = [fresh.launch_kind(k, counts=c) for k in (1, 8) for c in (False, True)]
    with golhip.Engine(SWITCH_W, SWITCH_H, k=8) as e:
        e.load(legs[0][0][0] * 255)
        for i, (rule, (gens, exp_counts)) in enumerate(zip(SWITCHES, legs)):
            assert alive(gens)
            e.set_rule(rule)
            kinds = [e.launch_kind(k, counts=c) for k in (1, 8) for c in (False, True)]
            assert kinds == (fresh_kinds if rule == LIFE else [kind_of(rule)] * 4), (i, kinds)
            counts = e.step(24, counts=True)
            assert e.turn == 24 * (i + 1)
            assert np.array_equal(i64(counts), exp_counts), (i, counts, exp_counts)
            assert np.array_equal(cells_of(e), gens[24]), i


def test_checkpoint_does_not_hold_the_rule(golhip, tmp_path):
    """include/golhip.h: a checkpoint holds the board and the turn, not the rule.  Saved under
    HighLife at turn 24 and loaded into a new handle, the board continues under B3/S23 until the
    caller sets the rule again; with it set, 8 more turns (<8, false, false, RuleConst<B36/S23>>) are
    HighLife's generation 32."""
    gens, _ = ref_of(SWITCH_W, SWITCH_H, HIGHLIFE, 32, guard_at=(24,))
    life8 = np_run(gens[24], LIFE, 8)[0][-1]
    assert alive([gens[24], life8]) and not np.array_equal(life8, gens[32])
    path = tmp_path / "highlife24.ckpt"
    with golhip.Engine(SWITCH_W, SWITCH_H, k=8, rule=HIGHLIFE) as e:
        e.load(gens[0] * 255)
        e.step(24)
        e.checkpoint_save(path)
    assert golhip.checkpoint_info(path) == (SWITCH_W, SWITCH_H, 24)
    with golhip.Engine(SWITCH_W, SWITCH_H, k=8) as e:
        assert e.rule == "B3/S23"
        e.checkpoint_load(path)
        assert e.rule == "B3/S23" and e.turn == 24
        assert np.array_equal(cells_of(e), gens[24])
        e.set_rule("B36/S23")
        assert e.launch_kind(8) == ("rule", 1)
        e.step(8)
        assert e.turn == 32
        got = cells_of(e)
        assert np.array_equal(got, gens[32]) and not np.array_equal(got, life8)
        e.checkpoint_load(path)  # the same checkpoint without setting the rule again is Life's
        e.set_rule("B3/S23")
        e.step(8)
        assert np.array_equal(cells_of(e), life8)
