"""The census without a GPU: golhip_batch_census is exported, declared and bound, the ABI version moved,
the header states the definitions, golhip.pattern / isolated / orientations / common_objects do what
they document (checked against brute force and a numpy B3/S23 step written here), the kernel's
translation unit is built and guarded against scratch, and the production library still passes the
boundary checks with it in."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import test_boundary
from conftest import PKG, ROOT

FUNCTION = "golhip_batch_census"


def test_library_exports_the_function(golhip):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / "lib" / "libgolhip.so")], text=True)
    exported = set(re.findall(r" T (golhip_\w+)", out))
    header = (ROOT / "include" / "golhip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*(golhip_\w+)\s*\(", header, re.M))
    assert FUNCTION in exported and FUNCTION in declared and FUNCTION in golhip.EXPORTS
    assert declared == set(golhip.EXPORTS) == exported
    lib = golhip.load_library()
    assert len(lib.golhip_batch_census.argtypes) == 5
    assert lib.golhip_version() >= 111  # 110: the exact search
    assert ctypes.sizeof(golhip.Pattern) == 264
    assert golhip.Pattern.alive.offset == 8 and golhip.Pattern.care.offset == 136


def test_the_header_states_the_definitions():
    header = " ".join((ROOT / "include" / "golhip.h").read_text().replace(" *", " ").split())
    for phrase in (
            "cell_i(x, y) is board i's cell.",
            "On a torus the coordinates are taken mod width and mod height.",
            "On a plane (golhip_batch_set_topology) a cell outside the rectangle is dead.",
            "Pattern p matches board i at anchor (x, y) when cell_i(x + c, y + r) == alive_p(r, c) for every (r, c) "
            "in care_p.",
            "Cells outside care_p are not looked at.",
            "On a torus: 0 <= x < width, 0 <= y < height.",
            "On a plane: -(w - 1) <= x <= width - 1 and -(h - 1) <= y <= height - 1.",
            "Every pattern has a live cell, so every match overlaps the board.",
            "An object touching the plane's border, with its dead ring outside, is counted.",
            "counts[i npat + p] is the number of matching anchors.",  # " *" is stripped above
            "Overlapping matches each count.",
            "residue[i] is the number of live cells of board i not covered by any match.",
            "A match (p, x, y) covers the cells (x + c, y + r) with alive_p(r, c) set, wrapped on a torus.",
            "With npat == 0, residue is golhip_batch_alive_counts's result and counts is not touched.",
            "npat < 0 or npat > 256", "patterns == NULL with npat > 0", "both outputs NULL",
            "w or h outside 1..32", "w > width or h > height", "a bit at column >= w, or in a row >= h",
            "alive not a subset of care", "a pattern without a live cell",
            "The rule plays no part.",
            "counts[.., p] does not depend on the other patterns.",
            "and the first golhip_batch_census (the pattern table: 66 KiB) allocates device memory"):
        assert phrase in header, phrase


def test_batch_has_the_interface(golhip):
    assert callable(golhip.Batch.census)
    doc = " ".join(golhip.Batch.census.__doc__.split())
    for word in ("anchor", "residue", "counts", "overlapping matches each count", "search_exact", "init_random",
                 "step(", "phase of the turn", "every phase", "-(w - 1) <= x <= width - 1"):
        assert word in doc, word


# --------------------------------------------------------------------------------- pattern()
def test_pattern_packs_the_bits(golhip):
    """3 rows of 5 cells with one cell not looked at, checked by hand: bit c of row r is column c."""
    p = golhip.pattern([[0, 1, 1, 0, 0],
                        [1, -1, 0, 0, 1],
                        [0, 0, 0, 1, 0]])
    assert (p.w, p.h) == (5, 3)
    assert list(p.alive)[:3] == [0b00110, 0b10001, 0b01000]
    assert list(p.care)[:3] == [0b11111, 0b11101, 0b11111]
    assert not any(list(p.alive)[3:]) and not any(list(p.care)[3:])
    full = golhip.pattern(np.ones((32, 32), dtype=np.int64))
    assert (full.w, full.h) == (32, 32) and set(full.alive) == {0xFFFFFFFF} and set(full.care) == {0xFFFFFFFF}


@pytest.mark.parametrize("cells,word", [
    (np.ones(3), "2-D"),
    (np.ones((2, 2, 2)), "2-D"),
    (np.ones((1, 33)), "1..32"),
    (np.ones((33, 1)), "1..32"),
    (np.ones((0, 3)), "1..32"),
    ([[0, 2], [1, 0]], "1 (alive), 0 (dead) or -1"),
    ([[0, 0], [0, 0]], "no live cell"),
    ([[-1, -1], [0, -1]], "no live cell"),
])
def test_pattern_refuses(golhip, cells, word):
    with pytest.raises(golhip.GolHipError) as e:
        golhip.pattern(cells)
    assert e.value.code == golhip.ERR_ARG and word in str(e.value)


# ------------------------------------------------------------------- isolated, orientations
def brute_orientations(a):
    """The set of the images of `a` under the 8 symmetries of the square, each written out by index."""
    a = np.asarray(a)
    h, w = a.shape
    images = set()
    for transpose in (False, True):
        for flip_r in (False, True):
            for flip_c in (False, True):
                hh, ww = (w, h) if transpose else (h, w)
                o = np.zeros((hh, ww), dtype=np.int8)
                for r in range(hh):
                    for c in range(ww):
                        rr, cc = (c, r) if transpose else (r, c)
                        if flip_r:
                            rr = h - 1 - rr
                        if flip_c:
                            cc = w - 1 - cc
                        o[r, c] = a[rr, cc]
                images.add((o.shape, o.tobytes()))
    return images


BLOCK = [[1, 1], [1, 1]]
BLINKER = [[1, 1, 1]]
BEEHIVE = [[0, 1, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0]]
GLIDER = [[0, 1, 0], [0, 0, 1], [1, 1, 1]]


@pytest.mark.parametrize("cells,n", [(BLOCK, 1), (BLINKER, 2), (BEEHIVE, 2), (GLIDER, 8)])
def test_orientations_are_the_distinct_images(golhip, cells, n):
    got = golhip.orientations(cells)
    assert len(got) == n
    assert np.array_equal(got[0], np.asarray(cells))  # the fixed order starts with the array itself
    as_set = {(o.shape, np.asarray(o, dtype=np.int8).tobytes()) for o in got}
    assert len(as_set) == n and as_set == brute_orientations(cells)
    again = golhip.orientations(cells)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_isolated_is_a_ring_of_dead_cells(golhip):
    iso = golhip.isolated(GLIDER)
    assert iso.shape == (5, 5)
    assert np.array_equal(iso[1:-1, 1:-1], np.asarray(GLIDER))
    ring = iso.copy()
    ring[1:-1, 1:-1] = 0
    assert not ring.any() and iso.sum() == 5
    p = golhip.pattern(iso)
    assert (p.w, p.h) == (5, 5) and list(p.care)[:5] == [31] * 5 and list(p.alive)[:5] == [0, 4, 8, 14, 0]


# --------------------------------------------------------------------------- common_objects
def life_step(a):
    """One B3/S23 generation on an unbounded plane: the array grows by one cell on every side."""
    a = np.pad(np.asarray(a, dtype=np.int64), 2)
    n = sum(np.roll(np.roll(a, dr, 0), dc, 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr, dc) != (0, 0))
    return (((a == 1) & ((n == 2) | (n == 3))) | ((a == 0) & (n == 3))).astype(np.int8)[1:-1, 1:-1]


def trimmed(a):
    """The bounding box of the live cells, and its top-left corner."""
    rows, cols = np.nonzero(a)
    return a[rows.min():rows.max() + 1, cols.min():cols.max() + 1], (rows.min(), cols.min())


EXPECTED = {"block": 1, "beehive": 2, "loaf": 4, "boat": 4, "tub": 1, "pond": 1, "ship": 2, "blinker": 2, "glider": 16}
CELLS = {"block": 4, "beehive": 6, "loaf": 7, "boat": 5, "tub": 4, "pond": 8, "ship": 6, "blinker": 3, "glider": 5}


def test_common_objects_is_the_catalogue(golhip):
    objs = golhip.common_objects()
    assert list(objs) == list(EXPECTED)
    assert {k: len(v) for k, v in objs.items()} == EXPECTED and sum(map(len, objs.values())) == 33
    everything = set()
    for name, arrays in objs.items():
        for a in arrays:
            a = np.asarray(a)
            assert set(np.unique(a)) <= {0, 1} and a.sum() == CELLS[name], name
            assert not a[0].any() and not a[-1].any() and not a[:, 0].any() and not a[:, -1].any(), name  # the ring
            assert a[1].any() and a[-2].any() and a[:, 1].any() and a[:, -2].any(), name  # and only one cell of it
            golhip.pattern(a)
            everything.add((a.shape, a.tobytes()))
        # every orientation of every array is in the list
        for a in arrays:
            assert brute_orientations(a) <= {(np.asarray(q).shape, np.asarray(q).tobytes()) for q in arrays}, name
    assert len(everything) == 33  # all distinct
    assert golhip.common_objects() is not objs  # data, built per call


def test_common_objects_behave_under_life(golhip):
    objs = golhip.common_objects()
    for name in ("block", "beehive", "loaf", "boat", "tub", "pond", "ship"):
        for a in objs[name]:
            nxt = life_step(a)
            assert np.array_equal(nxt[1:-1, 1:-1], a), name  # a fixed point, nothing born around it
            assert nxt.sum() == np.asarray(a).sum()
    b0, b1 = objs["blinker"]
    for src, dst in ((b0, b1), (b1, b0)):
        body, _ = trimmed(life_step(src))
        assert np.array_equal(body, trimmed(np.asarray(dst))[0])
    gliders = [trimmed(np.asarray(g)) for g in objs["glider"]]
    for g in objs["glider"]:
        body, (r, c) = trimmed(life_step(life_step(g)))
        r0, c0 = trimmed(np.asarray(g))[1]
        # two generations on, the array grew by 2 on every side: the body moved by (r - 2 - r0, c - 2 - c0)
        assert any(np.array_equal(body, q) for q, _ in gliders)
        assert sorted((abs(r - 2 - r0), abs(c - 2 - c0))) == [0, 1]  # half a diagonal step: one cell
        one = trimmed(life_step(g))[0]
        assert any(np.array_equal(one, q) for q, _ in gliders)  # every phase is in the list


# ---------------------------------------------------------------------------------- the build
def test_census_sources_are_in_the_build_and_the_scratch_guard():
    make = (PKG / "Makefile").read_text()
    csrc = PKG / "csrc"
    assert (csrc / "batch_census.hpp").exists() and (csrc / "batch_census.hip").exists()
    assert sorted(p.name for p in csrc.glob("batch_census*.hip")) == ["batch_census.hip"]  # one translation unit
    text = (csrc / "batch_census.hpp").read_text()
    assert text.count("__global__") == 1  # one kernel
    guard = [line for line in make.splitlines() if "--scratch-only" in line and "$(OUT)/stencil_board.o" in line]
    assert guard and all("$(BATCH_CENSUS_OBJS)" in line for line in guard)
    for kept in ("$(BATCH_RULE_OBJS)", "$(BATCH_PERIOD_OBJS)", "$(BATCH_SEARCH_OBJS)", "$(BATCH_PLANE_OBJS)",
                 "$(BATCH_CYCLE_OBJS)", "$(RULE_OBJS)", "$(OUT)/stencil_tile.o", "$(OUT)/batch_board.o",
                 "$(OUT)/stencil_slabq.o", "$(OUT)/view_kernels.o"):
        assert all(kept in line for line in guard), kept
    assert "csrc/batch_census.hpp" in [w for line in make.splitlines() if line.startswith("KDEPS") for w in line.split()]
    expanded = subprocess.check_output(["make", "-s", "-n", "-B", "-C", str(PKG), "guard"], text=True)
    guard_cmds = [line for line in expanded.splitlines() if "--scratch-only" in line and "stencil_board.o" in line]
    assert guard_cmds
    assert "csrc/batch_census.hip" in expanded  # compiled
    assert all("lib/batch_census.o" in line for line in guard_cmds)  # and guarded
    log = (PKG / "lib" / "vmcnt_guard.log")
    assert log.exists() and "0 use scratch" in log.read_text().splitlines()[-1]


def test_the_census_kernel_sits_in_its_own_translation_unit():
    csrc = PKG / "csrc"
    named = sorted(p.name for p in list(csrc.glob("*.hip")) + list(csrc.glob("*.hpp")) + list(csrc.glob("tuning/*"))
                   if "gol_batch_census" in p.read_text())
    assert named == ["batch_census.hip", "batch_census.hpp", "engine_batch.hip", "golhip_internal.hpp"]
    # the engine and the launch interface name it in comments; no other kernel translation unit does
    for p in csrc.glob("*.hip"):
        if p.name not in ("batch_census.hip", "engine_batch.hip"):
            assert "batch_census.hpp" not in p.read_text(), p.name


def test_production_sources_still_pass_the_boundary_checks(golhip):
    """The same checks as tests/test_boundary.py, run here because this change adds production
    sources (batch_census.hpp, batch_census.hip) and an export: no new environment hook, and the
    production library with the census kernel is still less than a third of the tuning library."""
    test_boundary.test_production_sources_never_name_the_tuning_build()
    test_boundary.test_production_library_reads_only_documented_hooks()
    test_boundary.test_library_exports_every_declared_symbol(golhip)
    test_boundary.test_tuning_library_exports_the_same_abi(golhip)
