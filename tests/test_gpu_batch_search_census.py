"""Batch.search_census (golhip_batch_search_census: the ash hand-off of gol_batch_cycle, csrc/batch_cycle.hpp,
then gol_batch_census over the chunk's ash): search_exact plus, per soup, the census of a board on the
soup's cycle, no boards kept.

Every comparison is exact.  The soups come from the existing path (init_random(seeds), store(), the
cells outside the soup box cleared); board(ash_turn) is numpy's, stepped from those cells
(search_census_cases.boards_at over np_step_boards / np_step_plane); the census is np_census of those
same boards; the records are search()'s and cycle_start is search_exact()'s, which their own tests
hold to the brute force.  The case table and the references live in tests/search_census_cases.py, and
tests/test_batch_search_census_cpu.py shows without a GPU that the cases meet the coverage conditions
asserted below."""
import ctypes

import numpy as np
import pytest

import search_census_cases as cases
from search_census_cases import HALF, LIFE, POSITION, POSITION_IDS, TOPOLOGIES, boards_at, box_mask, np_census
from test_gpu_batch_period import HIGHLIFE, STROBE, TABLE_RULE
from test_gpu_batch_search import soup_cells

pytestmark = pytest.mark.gpu


def fitting(golhip, h):
    """common_objects() as a list, without the arrays taller than the board (64 x 4: the library refuses
    them)."""
    return [p for p in cases.common_patterns(golhip) if p.shape[0] <= h]


_runs = {}  # (case, topology, density) -> everything one search_census call and its references gave


def run(golhip, case, topology, density_q32=HALF):
    key = (POSITION.index(case) if case in POSITION else case[:3] + (case[4],), topology, density_q32)
    if key not in _runs:
        w, h, box, seeds, max_turns = case
        seeds = np.array(seeds, dtype=np.uint64)
        cells = soup_cells(golhip, w, h, seeds, density_q32)
        if box is not None:
            cells = cells * box_mask(w, h, box)[None]
        pats = fitting(golhip, h)
        with golhip.Batch(w, h, 1, topology=topology, soup_box=box) as b:
            got = b.search_census(len(seeds), pats, seeds=seeds, density_q32=density_q32, max_turns=max_turns,
                                  ash=True)
            rec = b.search(len(seeds), seeds=seeds, density_q32=density_q32, max_turns=max_turns)
            rec2, start = b.search_exact(len(seeds), seeds=seeds, density_q32=density_q32, max_turns=max_turns)
        want = boards_at(cells, LIFE, got.ash_turn, topology == "plane")
        _runs[key] = dict(got=got, rec=rec, rec2=rec2, start=start, want=want, pats=pats, n=len(seeds))
    return _runs[key]


ALL_CASES = [(c, t) for c in POSITION for t in TOPOLOGIES]
ALL_IDS = [f"{i}-{t}" for i in POSITION_IDS for t in TOPOLOGIES]


# ---------------------------------------------------------------- 1. the position of every cell
@pytest.mark.parametrize("case,topology", ALL_CASES, ids=ALL_IDS)
def test_1_the_ash_is_board_ash_turn_cell_for_cell(golhip, case, topology):
    r = run(golhip, case, topology)
    got, n = r["got"], r["n"]
    w, h = case[:2]
    assert got.ash.dtype == np.uint8 and got.ash.shape == (n, h, w) and got.ash_turn.dtype == np.int64
    assert set(np.unique(got.ash)) <= {0, 1}
    repeated = got.records["repeat_turn"] >= 0
    assert 2 * int(repeated.sum()) >= n, got.records["repeat_turn"]
    assert (got.ash_turn[~repeated] == -1).all() and not got.ash[~repeated].any()
    for i in np.nonzero(repeated)[0]:
        assert np.array_equal(got.ash[i], r["want"][i]), (i, int(got.ash_turn[i]), got.records[i])
    assert got.ash[repeated].any()


def test_1_the_cases_cover_what_can_go_wrong(golhip):
    """ash_turn >= 512 somewhere (unrotate16 takes it mod 512); at width 512, where a row is not
    replicated, more than one lane rotation; a soup on its cycle at turn 0; a soup without a repeat."""
    turns = np.concatenate([run(golhip, c, t)["got"].ash_turn for c, t in ALL_CASES])
    assert (turns >= 512).any(), turns.max()
    for t in TOPOLOGIES:
        got = run(golhip, cases.WIDTH_512, t)["got"]
        rotations = {(int(v) // 32) % 16 for v in got.ash_turn[got.ash_turn >= 0]}
        assert len(rotations) >= 2, got.ash_turn
        r = run(golhip, cases.EMPTY, t, 0)
        got = r["got"]
        assert (got.cycle_start == 0).all() and (got.ash_turn == 0).all() and not got.ash.any()
        assert (got.records["repeat_turn"] == 1).all() and (got.residue == 0).all() and not got.counts.any()
        r = run(golhip, cases.TOO_SHORT, t)
        got = r["got"]
        lost = got.records["repeat_turn"] < 0
        assert lost.any() and (got.ash_turn[lost] == -1).all() and (got.cycle_start[lost] == -1).all()
        assert not got.ash[lost].any() and not got.counts[lost].any()
        assert np.array_equal(got.residue[lost], got.records["population"][lost]) and (got.residue[lost] > 0).all()
        assert np.array_equal(got.ash[~lost], r["want"][~lost])


# ---------------------------------------------------------------- 2. the census of those boards
@pytest.mark.parametrize("case,topology", ALL_CASES, ids=ALL_IDS)
def test_2_counts_and_residue_are_the_census_of_that_board(golhip, case, topology):
    r = run(golhip, case, topology)
    got = r["got"]
    assert got.counts.dtype == np.uint32 and got.counts.shape == (r["n"], len(r["pats"]))
    assert got.residue.dtype == np.uint32 and got.residue.shape == (r["n"],)
    counts, residue = np_census(r["want"], r["pats"], topology)
    lost = got.records["repeat_turn"] < 0
    residue = np.where(lost, got.records["population"].astype(np.int64), residue)
    assert not counts[lost].any()  # the reference boards of the soups without a repeat are dead
    assert np.array_equal(got.counts, counts), np.nonzero(got.counts != counts)
    assert np.array_equal(got.residue, residue), (got.residue, residue)


def test_2_some_board_holds_an_object_and_some_board_a_leftover(golhip):
    for t in TOPOLOGIES:
        seen = [run(golhip, c, t)["got"] for c in POSITION]
        assert any((g.counts[g.ash_turn >= 0] > 0).any() for g in seen)
        assert any((g.residue[g.ash_turn >= 0] > 0).any() for g in seen)


# ---------------------------------------------------------------- 3. records and cycle_start
@pytest.mark.parametrize("case,topology", ALL_CASES, ids=ALL_IDS)
def test_3_records_cycle_start_and_the_bounds(golhip, case, topology):
    r = run(golhip, case, topology)
    got, rec = r["got"], r["rec"]
    assert got.records.dtype == golhip.SOUP_DTYPE and got.records.tobytes() == rec.tobytes() == r["rec2"].tobytes()
    assert np.array_equal(got.cycle_start, r["start"])
    repeated = rec["repeat_turn"] >= 0
    assert ((got.cycle_start <= got.ash_turn) & (got.ash_turn <= rec["repeat_turn"]))[repeated].all()
    model = [golhip.search_census_turn(int(a), int(p), int(s))
             for a, p, s in zip(rec["repeat_turn"], rec["period"], got.cycle_start)]
    assert got.ash_turn.tolist() == model


# ---------------------------------------------------------------- 4. independence
def same(a, b):
    assert a.records.tobytes() == b.records.tobytes()
    for x, y in zip(a[1:], b[1:]):
        assert (x is None and y is None) or np.array_equal(x, y)


def test_4_outputs_do_not_depend_on_the_cuts_or_the_switches(golhip):
    n, max_turns = 24, 600
    pats = cases.common_patterns(golhip)
    with golhip.Batch(64, 32, 3, topology="plane", soup_box=(16, 16)) as b:
        b.init_random(seed0=5)
        b.track_period()
        b.step(70)
        before = (b.store(), b.turn, b.periods())
        whole = b.search_census(n, pats, seed0=900, max_turns=max_turns, ash=True)
        left = b.search_census(7, pats, seed0=900, max_turns=max_turns, ash=True)
        right = b.search_census(n - 7, pats, seed0=907, max_turns=max_turns, ash=True)
        glued = golhip.SearchCensus(*(np.concatenate([x, y]) for x, y in zip(left, right)))
        same(whole, glued)
        same(whole, b.search_census(n, pats, seeds=np.arange(900, 900 + n, dtype=np.uint64), max_turns=max_turns,
                                    ash=True))
        for off in ("counts", "residue", "ash"):
            kw = dict(counts=True, residue=True, ash=True)
            kw[off] = False
            part = b.search_census(n, pats, seed0=900, max_turns=max_turns, **kw)
            assert getattr(part, off) is None
            same(whole._replace(**{off: None}), part)
        only = b.search_census(n, [], seed0=900, max_turns=max_turns, counts=False, residue=True)
        assert np.array_equal(only.residue, np.where(whole.ash_turn >= 0, whole.ash.sum(axis=(1, 2)),
                                                     whole.records["population"]))
        after = (b.store(), b.turn, b.periods())
        assert before[1] == after[1] == 70 and np.array_equal(before[0], after[0])
        assert all(np.array_equal(x, y) for x, y in zip(before[2], after[2]))
        assert b.topology == "plane" and b.soup_box == (16, 16)
    assert (whole.counts > 0).any() and (whole.ash_turn > 0).any()


def test_4_a_stage_smaller_than_a_chunk(golhip, monkeypatch):
    """GOLHIP_STAGE_BYTES (read at create) caps the search's own stage as it caps the batch's: the census
    of a chunk then goes in groups of patterns and boards, the unpack row by row."""
    pats = cases.common_patterns(golhip)
    with golhip.Batch(64, 16, 1, soup_box=(16, 16)) as b:
        whole = b.search_census(20, pats, seed0=40, max_turns=600, ash=True)
    monkeypatch.setenv("GOLHIP_STAGE_BYTES", "100")
    with golhip.Batch(64, 16, 1, soup_box=(16, 16)) as b:
        same(whole, b.search_census(20, pats, seed0=40, max_turns=600, ash=True))


# ---------------------------------------------------------------- 5. the recipe
def test_5_init_random_step_census_reproduces_the_row(golhip):
    pats = cases.common_patterns(golhip)
    n = 24
    with golhip.Batch(64, 64, 1, topology="plane", soup_box=(16, 16)) as b:
        got = b.search_census(n, pats, seed0=400, max_turns=1100, ash=True)
    checked = 0
    for turn in sorted(set(got.ash_turn[got.ash_turn >= 0].tolist()))[:6]:
        idx = np.nonzero(got.ash_turn == turn)[0]
        with golhip.Batch(64, 64, len(idx), topology="plane", soup_box=(16, 16)) as look:
            look.init_random(seeds=(400 + idx).astype(np.uint64))
            look.step(int(turn))
            counts, residue = look.census(pats)
            assert np.array_equal(look.store() != 0, got.ash[idx] != 0)
        assert np.array_equal(counts, got.counts[idx]) and np.array_equal(residue, got.residue[idx])
        checked += len(idx)
    assert checked >= 6


# ---------------------------------------------------------------- 6. rules
def test_6_highlife_runs_the_table_form_of_the_pass(golhip):
    seeds = np.arange(24, dtype=np.uint64)
    cells = soup_cells(golhip, 64, 16, seeds)
    pats = cases.common_patterns(golhip)
    with golhip.Batch(64, 16, 2, rule=HIGHLIFE) as b:
        assert b.kernel_form == 1  # the search is constant-folded
        got = b.search_census(24, pats, seeds=seeds, max_turns=600, ash=True)
        rec, start = b.search_exact(24, seeds=seeds, max_turns=600)
    assert got.records.tobytes() == rec.tobytes() and np.array_equal(got.cycle_start, start)
    repeated = rec["repeat_turn"] >= 0
    assert repeated.any() and (got.ash_turn[repeated] > 0).any()
    want = boards_at(cells, HIGHLIFE, got.ash_turn, False)
    assert np.array_equal(got.ash, want)
    counts, residue = np_census(want, pats, "torus")
    residue = np.where(repeated, residue, rec["population"].astype(np.int64))
    assert np.array_equal(got.counts, counts) and np.array_equal(got.residue, residue)


def test_6_one_rule_per_soup(golhip):
    rng = np.random.default_rng(112)
    rules = [LIFE, HIGHLIFE, TABLE_RULE, STROBE] * 2 + [tuple(int(v) for v in rng.integers(0, 512, 2)) for _ in range(16)]
    seeds = np.full(len(rules), 17, dtype=np.uint64)
    cells = np.repeat(soup_cells(golhip, 64, 16, [17]) * box_mask(64, 16, (16, 16))[None], len(rules), axis=0)
    pats = cases.common_patterns(golhip)
    for topology in TOPOLOGIES:
        with golhip.Batch(64, 16, 1, topology=topology, soup_box=(16, 16)) as b:
            got = b.search_census(len(rules), pats, seeds=seeds, max_turns=300, rules=rules, ash=True)
            rec, start = b.search_exact(len(rules), seeds=seeds, max_turns=300, rules=rules)
        assert got.records.tobytes() == rec.tobytes() and np.array_equal(got.cycle_start, start)
        repeated = rec["repeat_turn"] >= 0
        assert repeated.sum() >= 4 and len(set(got.ash_turn.tolist())) >= 4, got.ash_turn
        want = boards_at(cells, rules, got.ash_turn, topology == "plane")
        assert np.array_equal(got.ash, want), topology
        counts, residue = np_census(want, pats, topology)
        residue = np.where(repeated, residue, rec["population"].astype(np.int64))
        assert np.array_equal(got.counts, counts) and np.array_equal(got.residue, residue)


# ---------------------------------------------------------------- 7. errors
def test_7_errors_leave_the_outputs_alone(golhip):
    lib = golhip.load_library()
    block = golhip.isolated([[1, 1], [1, 1]])
    table = (golhip.Pattern * 2)(golhip.pattern(block), golhip.Pattern(w=2, h=2))  # the second has no live cell
    with golhip.Batch(64, 16, 2) as b:
        b.init_random(seed0=3)
        b.step(5)
        boards = b.store()
        n = 4
        out = np.full(n, 7, dtype=golhip.SOUP_DTYPE)
        start = np.full(n, 77, dtype=np.int64)
        turn = np.full(n, 78, dtype=np.int64)
        counts = np.full((n, 2), 79, dtype=np.uint32)
        residue = np.full(n, 80, dtype=np.uint32)
        ash = np.full((n, 16, 64), 81, dtype=np.uint8)
        filled = [a.copy() for a in (out, start, turn, counts, residue, ash)]
        outs = (out.ctypes.data, start.ctypes.data, turn.ctypes.data)
        opt = (counts.ctypes.data, residue.ctypes.data, ash.ctypes.data)
        good = (ctypes.addressof(table), 1)
        calls = [
            ("a bad pattern", 300, (ctypes.addressof(table), 2), outs, opt, "pattern 1"),
            ("npat over 256", 300, (ctypes.addressof(table), 257), outs, opt, "257"),
            ("npat below 0", 300, (ctypes.addressof(table), -1), outs, opt, "-1"),
            ("patterns null", 300, (None, 1), outs, opt, "null"),
            ("all three optional outputs null", 300, good, outs, (None, None, None), "all null"),
            ("max_turns 0", 0, good, outs, opt, "max_turns"),
            ("max_turns above 2^20", (1 << 20) + 1, good, outs, opt, "max_turns"),
            ("counts without patterns", 300, (None, 0), outs, opt, "npat 0"),
            ("ash_turn null", 300, good, (outs[0], outs[1], None), opt, "ash_turn"),
        ]
        for what, max_turns, pats, req, optional, word in calls:
            rc = lib.golhip_batch_search_census(b._h, n, None, 0, HALF, max_turns, None, None, *pats, *req, *optional)
            assert rc == golhip.ERR_ARG, what
            assert word in lib.golhip_batch_last_error(b._h).decode(), (what, lib.golhip_batch_last_error(b._h))
            for a, f in zip((out, start, turn, counts, residue, ash), filled):
                assert np.array_equal(a, f), what
        with pytest.raises(golhip.GolHipError) as e:  # an array is refused before the library sees it
            b.search_census(n, [block, np.zeros((3, 3))], max_turns=300)
        assert e.value.code == golhip.ERR_ARG and "pattern 1" in str(e.value) and "no live cell" in str(e.value)
        with pytest.raises(golhip.GolHipError) as e:
            b.search_census(n, [block], max_turns=300, counts=False, residue=False)
        assert e.value.code == golhip.ERR_ARG
        with pytest.raises(golhip.GolHipError) as e:
            b.search_census(n, [np.pad(np.ones((1, 1), dtype=np.int8), ((16, 0), (0, 0)))], max_turns=300)
        assert e.value.code == golhip.ERR_ARG and "larger than" in str(e.value)
        # the handle is untouched, and a good call still works
        assert b.turn == 5 and np.array_equal(b.store(), boards)
        ok = b.search_census(n, [block], max_turns=300)
        assert ok.ash is None and ok.counts.shape == (n, 1) and (ok.ash_turn >= -1).all()
        empty = b.search_census(0, [block], max_turns=300, ash=True)
        assert empty.records.shape == (0,) and empty.counts.shape == (0, 1) and empty.ash.shape == (0, 16, 64)
