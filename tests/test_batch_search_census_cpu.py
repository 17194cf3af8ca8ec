"""The search census without a GPU: golhip_batch_search_census is exported, declared and bound, the ABI
version moved, the header, README and DESIGN state it, golhip.Batch has the interface, the cycle pass is
still the one translation unit tests/test_batch_cycle_cpu.py pins, the production library still passes
the boundary checks, search_census_turn is the documented function, and the cases of
tests/test_gpu_batch_search_census.py -- run here through the numpy references over the CPU oracle's
soups -- meet the conditions that test asserts on the GPU's results: they are not vacuous."""
import re
import subprocess

import numpy as np
import pytest

import search_census_cases as cases
import test_batch_cycle_cpu
import test_boundary
from conftest import PKG, ROOT

FUNCTION = "golhip_batch_search_census"


def test_library_exports_the_function(golhip):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / "lib" / "libgolhip.so")], text=True)
    exported = set(re.findall(r" T (golhip_\w+)", out))
    header = (ROOT / "include" / "golhip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*(golhip_\w+)\s*\(", header, re.M))
    assert FUNCTION in exported and FUNCTION in declared and FUNCTION in golhip.EXPORTS
    assert declared == set(golhip.EXPORTS) == exported
    lib = golhip.load_library()
    assert lib.golhip_version() >= 112  # 111: the census
    # b, nsoups, seeds, seed0, density, max_turns, birth, survive, patterns, npat, out, cycle_start, ash_turn,
    # counts, residue, ash_cells
    assert len(lib.golhip_batch_search_census.argtypes) == 16
    assert len(lib.golhip_batch_search_exact.argtypes) == 10 and len(lib.golhip_batch_census.argtypes) == 5


def test_the_declaration_is_the_signature():
    header = " ".join(re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "golhip.h").read_text(), flags=re.S).split())
    m = re.search(r"int golhip_batch_search_census\((.*?)\);", header)
    assert m
    names = [arg.split()[-1].lstrip("*") for arg in m.group(1).split(",")]
    assert names == ["b", "nsoups", "seeds", "seed0", "density_q32", "max_turns", "birth", "survive", "patterns", "npat",
                     "out", "cycle_start", "ash_turn", "counts", "residue", "ash_cells"]
    source = " ".join((PKG / "csrc" / "engine_batch.hip").read_text().split())
    d = re.search(r"int golhip_batch_search_census\((.*?)\) \{", source)
    assert d and [arg.split()[-1].lstrip("*") for arg in d.group(1).split(",")] == names


def test_the_header_states_the_contract():
    header = " ".join((ROOT / "include" / "golhip.h").read_text().replace(" *", " ").split())
    for phrase in ("out is byte for byte what golhip_batch_search writes for the same arguments and cycle_start is "
                   "what golhip_batch_search_exact writes",
                   "cycle_start <= ash_turn <= repeat_turn",
                   "no generation beyond repeat_turn has run",
                   "it is NOT aligned to cycle_start's phase",
                   "golhip_batch_init_random with the soup's seed, golhip_batch_step(ash_turn)",
                   "0 or 1.",
                   "may be NULL, not all three",
                   "npat == 0 is allowed when counts is NULL",
                   "ash_turn -1, a counts row of zeros, ash_cells all dead and residue = the record's population",
                   "all before any device work",
                   "the batch's boards, turn, rules, records, switches, topology and box all stay",
                   "at or below 64 MiB: 65536 soups of 64 x 64, 2048 of 512 x 512",
                   "the first golhip_batch_search_census"):
        assert phrase in header, phrase


def test_batch_has_the_interface(golhip):
    assert callable(golhip.Batch.search_census)
    assert golhip.SearchCensus._fields == ("records", "cycle_start", "ash_turn", "counts", "residue", "ash")
    doc = " ".join(golhip.Batch.search_census.__doc__.split())
    for word in ("init_random(seeds=[seed])", "step(ash_turn)", "same soup_box and topology", "cycle_start <= ash_turn",
                 "-1", "population", "every phase"):
        assert word in doc, word
    assert "search_census()" in " ".join(golhip.Batch.census.__doc__.split())


def test_the_documents_have_the_section():
    design = (ROOT / "DESIGN.md").read_text()
    assert re.search(r"^#+ 3\.14\b.*search_census", design, re.M)
    section = design[design.index("3.14"):]
    for word in ("golhip_batch_search_census", "ash_turn", "barrier", "unrotate16", "slack", "Not measured"):
        assert word in section, word
    assert "search_census" in (ROOT / "README.md").read_text()
    assert "golhip_batch_search_census" in (ROOT / "INTEGRATION.md").read_text()


def test_the_cycle_sources_are_what_they_were_pinned_to():
    test_batch_cycle_cpu.test_batch_cycle_sources_are_in_the_build_and_the_scratch_guard()
    test_batch_cycle_cpu.test_the_exact_pass_leaves_the_other_kernel_sources_alone()
    text = (PKG / "csrc" / "batch_cycle.hpp").read_text()
    assert text.count("__global__") == 1  # the hand-off is a tail of the one kernel, not a kernel
    assert "cp.ash" in text and "unrotate16(a[r], tl, T & 511)" in text
    internal = (PKG / "csrc" / "golhip_internal.hpp").read_text()
    params = internal[internal.index("struct BatchCycleParams"):]
    params = params[:params.index("};")]
    assert "uint32_t *ash;" in params and "int64_t *ash_turn;" in params


def test_production_sources_still_pass_the_boundary_checks(golhip):
    test_boundary.test_production_sources_never_name_the_tuning_build()
    test_boundary.test_production_library_reads_only_documented_hooks()
    test_boundary.test_library_exports_every_declared_symbol(golhip)
    test_boundary.test_tuning_library_exports_the_same_abi(golhip)


# ------------------------------------------------------------------------- search_census_turn
def pass_turn(repeat_turn, period, cycle_start):
    """gol_batch_cycle's counters, written out as a loop: the turn of board A when the pass stops."""
    if repeat_turn < 0:
        return -1
    s = repeat_turn - period
    if s <= 0:
        return 0
    half = (s + 1) >> 1
    lo = half - 1 if period <= half else 0
    n = s - lo + 1
    turn, i, stop, pending = lo + period, 0, False, None
    while i < n - 1:
        turn += 1  # index i compares, then steps
        if pending is not None:  # wave 0 takes the block put one index earlier
            stop = stop or cycle_start - lo < 32 * pending + 32
            pending = None
        if i % 32 == 31:
            pending = i // 32
        if i % 32 == 1 and stop:
            return turn
        i += 1
    return turn


def test_search_census_turn_is_the_pass(golhip):
    f = golhip.search_census_turn
    assert f(-1, -1, -1) == -1 and f(1, 1, 0) == 0 and f(2, 2, 0) == 0
    assert f(3, 2, 0) == 3  # a blinker soup: noticed from the snapshot of turn 1, the closing compare
    for j in range(0, 13):
        s = (1 << j) - 1
        for p in sorted({1, 2, 3, 30, (1 << j) // 2, (1 << j) // 2 + 1, 1 << j} - {0}):
            if p > 1 << j:
                continue
            lo = golhip.cycle_start_floor(s + p, p)
            for start in sorted({lo, lo + 1, lo + 31, lo + 32, lo + 33, (lo + s) // 2, s - 34, s - 33, s - 2, s - 1, s}):
                if not lo <= start <= s or (lo > 0 and start == lo):
                    continue  # cycle_start is above a floor that is a snapshot turn
                t = f(s + p, p, start)
                assert t == pass_turn(s + p, p, start), (j, p, start)
                assert start <= t <= s + p, (j, p, start, t)
                assert s == 0 or t >= lo + p


# ------------------------------------------------------------------------- the cases are not vacuous
def run_case(golhip, oracle, case, plane, density_q32=cases.HALF):
    w, h, box, seeds, max_turns = case
    cells = cases.oracle_cells(oracle, w, h, seeds, box, density_q32)
    return cells, cases.reference(golhip, cells, cases.LIFE, max_turns, plane)


@pytest.mark.parametrize("plane", [False, True], ids=cases.TOPOLOGIES)
def test_the_whole_board_soups_run_past_turn_512(golhip, oracle, plane):
    _, (rep, _, start, turn, boards) = run_case(golhip, oracle, cases.WHOLE_BOARD, plane)
    assert (turn >= 512).any(), turn
    assert ((start <= turn) & (turn <= rep))[rep >= 0].all()
    assert boards[turn >= 512].any()  # and the ash there is not the empty board


@pytest.mark.parametrize("plane", [False, True], ids=cases.TOPOLOGIES)
def test_width_512_turns_the_lanes_by_more_than_one_amount(golhip, oracle, plane):
    """unrotate16 moves a row by (ash_turn / 32) mod 16 lanes at width 512: two amounts at the least."""
    _, (rep, _, _, turn, _) = run_case(golhip, oracle, cases.WIDTH_512, plane)
    assert len({(int(t) // 32) % 16 for t in turn[rep >= 0]}) >= 2, turn
    assert len({int(t) % 32 for t in turn[rep >= 0]}) >= 2, turn


@pytest.mark.parametrize("plane", [False, True], ids=cases.TOPOLOGIES)
def test_the_empty_and_the_short_case(golhip, oracle, plane):
    _, (rep, period, start, turn, boards) = run_case(golhip, oracle, cases.EMPTY, plane, density_q32=0)
    assert (rep == 1).all() and (period == 1).all() and (start == 0).all() and (turn == 0).all() and not boards.any()
    _, (rep, _, start, turn, boards) = run_case(golhip, oracle, cases.TOO_SHORT, plane)
    assert (rep < 0).any() and ((start < 0) == (rep < 0)).all() and ((turn < 0) == (rep < 0)).all()
    assert not boards[rep < 0].any()


@pytest.mark.parametrize("plane", [False, True], ids=cases.TOPOLOGIES)
def test_the_census_of_a_case_sees_objects_and_leftovers(golhip, oracle, plane):
    """64 x 64 with 16 x 16 soups: some board holds a listed object, some board a cell the list does not
    explain (an oscillator in a phase of its own, or an object the list does not hold)."""
    case = cases.POSITION[4]
    assert case[:3] == (64, 64, (16, 16))
    _, (rep, _, _, turn, boards) = run_case(golhip, oracle, case, plane)
    counts, residue = cases.np_census(boards, cases.common_patterns(golhip), cases.TOPOLOGIES[plane])
    assert (rep >= 0).sum() >= 6
    assert (counts > 0).any() and (residue > 0).any(), (counts.sum(axis=0), residue)
    # a translated board has the same census on a torus: the counts cannot see a wrong position
    if not plane:
        moved = np.roll(boards, (3, 5), axis=(1, 2))
        c2, r2 = cases.np_census(moved, cases.common_patterns(golhip), "torus")
        assert np.array_equal(c2, counts) and np.array_equal(r2, residue) and not np.array_equal(moved, boards)
