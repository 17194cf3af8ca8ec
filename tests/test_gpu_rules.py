"""Life-like rules on the GPU (golhip_set_rule, the rule-generic streaming kernel gol_rule of
csrc/golhip_rule.hpp): every rule but B3/S23 runs gol_rule -- constant-folded for the catalogue
(HighLife, Day & Night, Seeds, Replicator), the table form for every other rule -- through single
strips, multi-strip handles, per-turn counts, the flips ring, flip tracking and the host CLI.

The oracle is B3/S23 only, so the reference is the numpy stepper below (eight rolls summed, then
where(alive, survive >> n & 1, birth >> n & 1)); everything is bit-exact.  tests/test_rules_cpu.py
checks that stepper against the oracle at B3/S23, and the kernel's algebra without a GPU.
tests/test_gpu_rules_matrix.py runs every functor at every depth with and without counts and flips,
boards down to one row, strips that take the K = 8 interior + boundary split, rank mode as the RCCL
ring of one, rule changes at depth and the checkpoint; tests/test_gpu_rank_host.py runs two real
ranks under AntiLife over both transports.
"""
import functools
import subprocess

import numpy as np
import pytest

from conftest import PKG, REF

pytestmark = pytest.mark.gpu

HIGHLIFE = (0x048, 0x00C)                     # B36/S23, constant-folded
TABLE_RULE = (0x108, 0x04D)                   # B38/S0236, table form
ANTILIFE = (0x19F, 0x1DF)                     # B0123478/S01234678
CATALOGUE = [HIGHLIFE, (0x1C8, 0x1D8), (0x004, 0x000), (0x0AA, 0x0AA)]


def np_step(cells, rule):
    """One generation of a 0/1 torus board under (birth, survive)."""
    birth, survive = rule
    c = cells.astype(np.int64)
    n = sum(np.roll(np.roll(c, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    return np.where(cells == 1, (survive >> n) & 1, (birth >> n) & 1).astype(np.uint8)


def np_run(cells, rule, turns):
    """(generations 0..turns as a list, counts of generations 1..turns)."""
    gens = [cells]
    for _ in range(turns):
        gens.append(np_step(gens[-1], rule))
    return gens, np.array([int(g.sum()) for g in gens[1:]], dtype=np.int64)


def random_cells(w, h, seed, density=0.5):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reference(w, h, seed, rule, turns):
    return np_run(random_cells(w, h, seed), rule, turns)


def flips_of(a, b):
    ys, xs = np.nonzero(a != b)
    return np.stack([xs, ys], 1).astype(np.int32)


def cells_of(e):
    return (e.store() != 0).astype(np.uint8)


# ---------------------------------------------------------------- 1. truth tables
def truth_rules():
    rng = np.random.default_rng(7)
    named = CATALOGUE + [(0x008, 0x00C), (0, 0), (0x1FF, 0x1FF), ANTILIFE]
    return named + [tuple(int(v) for v in rng.integers(0, 512, 2)) for _ in range(64)]


def test_truth_tables(golhip):
    """One generation of one dense board -- it holds every (state, neighbour count) combination --
    under the catalogue, B3/S23 set explicitly, the empty and the full rule, AntiLife and 64 seeded
    random rules, on one engine; kind 5 with the catalogue / table split, B3/S23 as a fresh engine."""
    cells = random_cells(128, 64, 1)
    c = cells.astype(np.int64)
    n = sum(np.roll(np.roll(c, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    for state in (0, 1):
        for k in range(9):
            assert np.count_nonzero((cells == state) & (n == k)) >= 10, (state, k)
    with golhip.Engine(128, 64, k=8) as fresh:
        life_kind = fresh.launch_kind(8), fresh.launch_kind(8, counts=True)
    with golhip.Engine(128, 64, k=8) as e:
        assert e.rule == "B3/S23" and e.rule_masks == (0x008, 0x00C)
        for rule in truth_rules():
            e.set_rule_masks(*rule)
            assert e.rule_masks == rule and golhip.parse_rule(e.rule) == rule
            if rule == (0x008, 0x00C):
                assert (e.launch_kind(8), e.launch_kind(8, counts=True)) == life_kind
            else:
                want = ("rule", 1 if rule in CATALOGUE else 0)
                assert e.launch_kind(8) == want and e.launch_kind(1, counts=True) == want, rule
            e.load(cells * 255)
            counts = e.step(1, counts=True)
            exp = np_step(cells, rule)
            assert np.array_equal(cells_of(e), exp), golhip.rule_string(*rule)
            assert int(counts[0]) == int(exp.sum()), golhip.rule_string(*rule)


# ---------------------------------------------------------------- 2. geometry
GEOMETRY = [
    (16, 16, None),        # L = 128, replicated, height < 2K
    (48, 37, None),        # L = 384, odd height
    (2048, 40, None),      # wd = 64: two column chunks, the last holding 2 words
    (4000, 24, None),      # L = 16000: a ragged last chunk
    (2048, 40, "bands8"),  # five bands
    (2048, 40, "tail"),    # graded bands
]


@pytest.mark.parametrize("w,h,mode", GEOMETRY)
@pytest.mark.parametrize("rule", [HIGHLIFE, TABLE_RULE], ids=["const", "table"])
def test_geometry(golhip, w, h, mode, rule):
    """23 turns (8 + 8 + 4 + 2 + 1 at k = 8) with the count of every turn, each rule depth alone via
    set_k + set_fixed_k."""
    gens, exp_counts = reference(w, h, w + h, rule, 23)
    with golhip.Engine(w, h, k=8, rule=rule) as e:
        if mode == "bands8":
            e.set_band_rows(8)
        elif mode == "tail":
            e.set_tail_bands(2, 4)
        e.set_fixed_k(True)
        for depth in (8, 4, 2, 1):
            e.set_k(depth)
            assert e.launch_kind(depth, counts=True) == ("rule", 1 if rule == HIGHLIFE else 0)
            e.load(gens[0] * 255)
            counts = e.step(23, counts=True)
            assert np.array_equal(counts.astype(np.int64), exp_counts), (depth, counts, exp_counts)
            assert np.array_equal(cells_of(e), gens[23]), depth
            e.load(gens[0] * 255)
            e.step(23)  # the launches without counts are other kernels
            assert np.array_equal(cells_of(e), gens[23]), depth


# ---------------------------------------------------------------- 3. strips
@pytest.mark.parametrize("rule", [HIGHLIFE, TABLE_RULE], ids=["const", "table"])
def test_strips(golhip, rule):
    """Uneven 17 / 17 / 16 row strips in halo mode: the same board and counts as one strip."""
    gens, exp_counts = reference(2048, 50, 3, rule, 23)
    with golhip.Engine(2048, 50, ngpus=1, k=8, strips=3, rule=rule) as e:
        assert e.launch_kind(8)[0] == "rule"
        e.load(gens[0] * 255)
        counts = e.step(23, counts=True)
        got = cells_of(e)
    with golhip.Engine(2048, 50, k=8, rule=rule) as e:
        e.load(gens[0] * 255)
        single_counts = e.step(23, counts=True)
        single = cells_of(e)
    assert np.array_equal(counts.astype(np.int64), exp_counts)
    assert np.array_equal(got, gens[23])
    assert np.array_equal(single, got) and np.array_equal(single_counts, counts)


# ---------------------------------------------------------------- 4. flips
@pytest.mark.parametrize("w,h", [(64, 64), (2048, 40)])
@pytest.mark.parametrize("rule", [HIGHLIFE, TABLE_RULE], ids=["const", "table"])
def test_flips(golhip, w, h, rule):
    gens, exp_counts = reference(w, h, 5, rule, 24)
    with golhip.Engine(w, h, k=8, rule=rule) as e:
        e.load(gens[0] * 255)
        per_turn, alive = e.step_flips(12, counts=True)
        assert np.array_equal(alive.astype(np.int64), exp_counts[:12])
        for t in range(12):
            assert np.array_equal(per_turn[t], flips_of(gens[t], gens[t + 1])), t
        x, offs, alive = e.step_flips_rows(12, counts=True)
        assert np.array_equal(alive.astype(np.int64), exp_counts[12:24])
        rows = golhip.Engine.rows_to_cells(x, offs, h, 12)
        for t in range(12):
            assert np.array_equal(rows[t], flips_of(gens[12 + t], gens[13 + t])), t
        assert e.turn == 24
        e.load(gens[0] * 255)
        e.track_flips(True)
        e.step(8)
        assert np.array_equal(e.flips(), flips_of(gens[7], gens[8]))
        assert np.array_equal(cells_of(e), gens[8])


# ---------------------------------------------------------------- 5. AntiLife against the oracle
def test_antilife_is_the_complement_of_life(golhip, oracle):
    """The complement of a board under B0123478/S01234678 is the complement of Life: a B0 rule on
    the replica-padded torus, against the project's oracle."""
    w, h, turns = 512, 96, 40
    board = random_cells(w, h, 13, 0.4)
    ref, life_counts = oracle.packed_run(board * 255, turns)
    with golhip.Engine(w, h, k=8, rule="B0123478/S01234678") as e:
        assert e.rule_masks == ANTILIFE and e.launch_kind(8) == ("rule", 0)
        e.load((1 - board) * 255)
        counts = e.step(turns, counts=True)
        got = cells_of(e)
    assert np.array_equal(got, 1 - (ref != 0).astype(np.uint8))
    assert np.array_equal(counts.astype(np.int64), w * h - life_counts)


# ---------------------------------------------------------------- 6. rule changes and caches
def test_rule_changes_drop_the_caches(golhip, oracle):
    """Graph replays on, 300 turns each of B3/S23, HighLife and B3/S23 again on one handle: the board
    and the turn at each switch, and B3/S23's launch kinds after the last one as on a fresh engine."""
    _, _, img = oracle.read_pgm(REF / "images" / "64x64.pgm")
    cells = (img != 0).astype(np.uint8)
    life = (0x008, 0x00C)
    with golhip.Engine(64, 64, k=16) as fresh:
        fresh_kinds = [fresh.launch_kind(k, counts=c) for k in (1, 8, 16) for c in (False, True)]
    with golhip.Engine(64, 64, k=16) as e:
        e.set_graphs(1)
        e.load(cells * 255)
        for i, rule in enumerate([life, HIGHLIFE, life]):
            e.set_rule(golhip.rule_string(*rule))
            counts = e.step(300, counts=True)
            gens, exp_counts = np_run(cells, rule, 300)
            cells = gens[-1]
            assert e.turn == 300 * (i + 1)
            assert np.array_equal(cells_of(e), cells), i
            assert np.array_equal(counts.astype(np.int64), exp_counts), i
        assert [e.launch_kind(k, counts=c) for k in (1, 8, 16) for c in (False, True)] == fresh_kinds


# ---------------------------------------------------------------- 7. refusals
def test_persistent_refuses_other_rules(golhip, oracle):
    with golhip.Engine(4096, 4096, k=16, rule="B36/S23") as e:
        e.init_random(3)
        e.step(3)
        before = oracle.digest_words(e.store_words())
        with pytest.raises(golhip.GolHipError) as err:
            e.step_persistent(64)
        assert err.value.code == golhip.ERR_STATE and "B3/S23" in str(err.value)
        assert e.turn == 3
        assert oracle.digest_words(e.store_words()) == before


def test_bad_rule_leaves_the_handle_untouched(golhip):
    cells = random_cells(64, 64, 9)
    with golhip.Engine(64, 64, k=8, rule="B36/S23") as e:
        e.load(cells * 255)
        with pytest.raises(golhip.GolHipError) as err:
            e.set_rule("B9/S")
        assert err.value.code == golhip.ERR_ARG and "B9/S" in str(err.value)
        with pytest.raises(golhip.GolHipError) as err:
            e.set_rule((0x200, 0))
        assert err.value.code == golhip.ERR_ARG
        assert e.rule == "B36/S23"
        e.step(5)
        assert np.array_equal(cells_of(e), np_run(cells, HIGHLIFE, 5)[0][-1])
    with pytest.raises(golhip.GolHipError):
        golhip.Engine(64, 64, rule="nonsense")


def test_board_kernel_setting_is_bypassed(golhip):
    gens, exp_counts = reference(64, 64, 21, HIGHLIFE, 30)
    with golhip.Engine(64, 64, k=16) as e:
        e.set_board_kernel(1)
        e.set_activity(1)
        assert e.launch_kind(16)[0] == "board"
        e.set_rule("B36/S23")
        assert e.launch_kind(16) == ("rule", 1)
        e.load(gens[0] * 255)
        counts = e.step(30, counts=True)
        assert np.array_equal(counts.astype(np.int64), exp_counts)
        assert np.array_equal(cells_of(e), gens[30])


# ---------------------------------------------------------------- 8. host
def test_cli_rule(tmp_path, oracle):
    gol = PKG / "lib" / "gol"
    p = subprocess.run([str(gol), "-rule", "B36/S23", "-w", "64", "-h", "64", "-turns", "50", "-noVis", "-images",
                        str(REF / "images"), "-out", str(tmp_path)],
                       stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    _, _, img = oracle.read_pgm(REF / "images" / "64x64.pgm")
    exp = np_run((img != 0).astype(np.uint8), HIGHLIFE, 50)[0][-1]
    _, _, got = oracle.read_pgm(tmp_path / "64x64x50.pgm")
    assert np.array_equal((got != 0).astype(np.uint8), exp)
    assert not np.array_equal(exp * 255, oracle.packed_run(img, 50)[0])  # HighLife, not Life
    bad = subprocess.run([str(gol), "-rule", "nonsense", "-w", "64", "-h", "64", "-turns", "5", "-noVis", "-images",
                          str(REF / "images"), "-out", str(tmp_path)],
                         stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "nonsense" in bad.stderr
