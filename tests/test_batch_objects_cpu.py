"""The objects without a GPU: golhip_batch_objects and golhip_batch_search_objects are exported, declared and
bound, the ABI version moved, the header states the definitions, the new translation unit is compiled
and on the scratch guard, the production library still passes the boundary checks with the new kernel
in, object_hash is the hash of the definitions, and the case table of tests/objects_cases.py is complete
and not vacuous: np_objects itself meets each family's conditions."""
import re
import subprocess

import numpy as np
import pytest

import objects_cases as cases
import test_boundary
from conftest import PKG, ROOT
from objects_cases import AT_BORDER, WINDS_X, WINDS_Y

FUNCTIONS = ("golhip_batch_objects", "golhip_batch_search_objects")


def test_library_exports_the_functions(golhip):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / "lib" / "libgolhip.so")], text=True)
    exported = set(re.findall(r" T (golhip_\w+)", out))
    declared = set(test_boundary.header_functions())
    for f in FUNCTIONS:
        assert f in exported and f in declared and f in golhip.EXPORTS
    assert declared == set(golhip.EXPORTS) == exported
    lib = golhip.load_library()
    assert lib.golhip_version() >= 113  # 112: the search census
    assert len(lib.golhip_batch_objects.argtypes) == 5 and len(lib.golhip_batch_search_objects.argtypes) == 15
    assert golhip.OBJECT_DTYPE.itemsize == 32 and golhip.OBJECT_DTYPE == cases.OBJECT_DTYPE
    assert golhip.OBJECT_DTYPE.names == ("x", "y", "w", "h", "population", "flags", "hash")
    assert golhip.SearchObjects._fields == ("records", "cycle_start", "ash_turn", "nobjects", "objects")
    assert callable(golhip.Batch.objects) and callable(golhip.Batch.search_objects)
    assert (golhip.OBJECT_WINDS_X, golhip.OBJECT_WINDS_Y, golhip.OBJECT_AT_BORDER) == (WINDS_X, WINDS_Y, AT_BORDER)


def test_the_declarations_are_the_signatures():
    header = " ".join(re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "golhip.h").read_text(), flags=re.S).split())
    source = " ".join((PKG / "csrc" / "engine_batch.hip").read_text().split())
    want = {"golhip_batch_objects": ["b", "max_objects", "reach", "nobjects", "objects"],
            "golhip_batch_search_objects": ["b", "nsoups", "seeds", "seed0", "density_q32", "max_turns", "birth", "survive",
                                            "max_objects", "reach", "out", "cycle_start", "ash_turn", "nobjects", "objects"]}
    for f, names in want.items():
        m = re.search(r"int %s\((.*?)\);" % f, header)
        assert m and [arg.split()[-1].lstrip("*") for arg in m.group(1).split(",")] == names
        d = re.search(r"int %s\((.*?)\) \{" % f, source)
        assert d and [arg.split()[-1].lstrip("*") for arg in d.group(1).split(",")] == names
    assert "} golhip_object_t;" in header and "uint64_t hash;" in header


def test_the_header_states_the_definitions():
    header = " ".join((ROOT / "include" / "golhip.h").read_text().replace(" *", " ").split())
    for phrase in ("Two live cells of a board are linked when their Chebyshev distance is at most reach",
                   "On a torus the distance is taken mod width and mod height",
                   "A cluster is a connected component of that relation",
                   "numbered by their first cell in row-major order: smallest y, then smallest x",
                   "at most one cyclic run of empty columns of length >= reach",
                   "x0 is the column just after it",
                   "x0 = 0, w = width, and flag WINDS_X is set",
                   "A single cell on a torus of width <= reach winds by this rule",
                   "dx = (x - x0) mod width, dy = (y - y0) mod height",
                   "z = v + 0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB",
                   "7 h-1-dy w-1-dx h x w",
                   "mix(v<<16 | u), mod 2^64) XOR mix(1<<32 | oh<<16 | ow)",
                   "hash is the smallest H_k as an unsigned number",
                   "A winding cluster's hash depends on its position along the winding axis",
                   "golhip_object_t is 32 bytes",
                   "Bit 2 is AT_BORDER. It is set only on a plane",
                   "also when it exceeds max_objects", "The rest are left untouched",
                   "all checks come before any device work",
                   "the cap only cuts the list"):
        assert phrase in header, phrase


def test_the_translation_unit_is_compiled_and_guarded():
    make = (PKG / "Makefile").read_text()
    assert "csrc/batch_objects.hip" in make and "csrc/batch_objects.hpp" in make
    assert "BATCH_OBJECTS_OBJS := $(OUT)/batch_objects.o" in make
    guard = [line for line in make.splitlines() if "--scratch-only" in line and "$(OUT)/stencil_tile.o" in line]
    assert len(guard) == 1 and "$(BATCH_OBJECTS_OBJS)" in guard[0]
    rule = [line for line in make.splitlines() if line.startswith("$(OUT)/vmcnt_guard.ok:")]
    assert len(rule) == 1 and "$(BATCH_OBJECTS_OBJS)" in rule[0]
    # only the production library is linked without its local symbols
    links = [line for line in make.splitlines() if "-shared" in line]
    assert len(links) == 3 and [("--strip-all" in line) for line in links] == [True, False, False]
    header = (PKG / "csrc" / "batch_objects.hpp").read_text()
    assert re.findall(r'#include "(.*?)"', header) == ["golhip_internal.hpp"]
    assert header.count("__global__") == 1 and "The barrier argument" in header
    assert (PKG / "lib" / "batch_objects.o").exists()
    log = (PKG / "lib" / "vmcnt_guard.log").read_text().strip().splitlines()
    assert re.fullmatch(r"check_vmcnt --scratch-only: \d+ kernels checked, 0 use scratch", log[-1]), log[-1]


def test_production_library_still_passes_the_boundary_checks(golhip):
    """The size test among them, with gol_batch_objects linked in."""
    test_boundary.test_production_sources_never_name_the_tuning_build()
    test_boundary.test_production_library_reads_only_documented_hooks()
    test_boundary.test_library_exports_every_declared_symbol(golhip)
    test_boundary.test_library_is_gfx950_code(golhip)
    test_boundary.test_tuning_library_exports_the_same_abi(golhip)
    prod = (PKG / "lib" / "libgolhip.so").stat().st_size
    tuning = (PKG / "lib_tuning" / "libgolhip.so").stat().st_size
    assert tuning - 3 * prod >= 64 * 1024, (prod, tuning)  # room to spare, not a few bytes


def test_the_documents_have_the_section():
    design = (ROOT / "DESIGN.md").read_text()
    assert re.search(r"^#+ 3\.15\b.*gol_batch_objects", design, re.M)
    section = design[design.index("3.15"):]
    for word in ("golhip_batch_objects", "golhip_batch_search_objects", "barrier", "--strip-all", "slack", "objects compared",
                 "Not measured", "Out of scope"):
        assert word in section, word
    readme = " ".join((ROOT / "README.md").read_text().split())
    assert "Batch.objects" in readme and "common_object_hashes()" in readme and "np.unique" in readme


# ------------------------------------------------------------------------------ object_hash
def shapes_under_test(golhip):
    shapes = {name: arrays[0][1:-1, 1:-1] for name, arrays in golhip.common_objects().items()}
    shapes["glider-phase-2"] = golhip.common_objects()["glider"][8][1:-1, 1:-1]
    rng = np.random.default_rng(15)
    while len(shapes) < 10 + 50:
        a = (rng.random((5, 5)) < 0.5).astype(np.int8)
        if a.any():
            shapes[f"random-{len(shapes)}"] = a
    return shapes


def trimmed(a):
    ys, xs = np.nonzero(a)
    return a[ys.min():ys.max() + 1, xs.min():xs.max() + 1]


def canonical(a):
    return min((o.shape, o.tobytes()) for o in [np.ascontiguousarray(x) for x in eight(trimmed(a))])


def eight(a):
    return [np.rot90(b, k) for b in (a, np.fliplr(a)) for k in range(4)]


def test_object_hash_does_not_change_under_the_eight_orientations_and_translation(golhip):
    shapes = shapes_under_test(golhip)
    assert len(shapes) == 60
    keys = {}
    for name, a in shapes.items():
        h = golhip.object_hash(a)
        assert 0 <= h < 1 << 64
        for o in eight(a):
            assert golhip.object_hash(o) == h, name
            assert golhip.object_hash(np.pad(o, ((3, 1), (0, 7)))) == h, name
        keys.setdefault(canonical(a), set()).add(h)
    assert all(len(v) == 1 for v in keys.values())
    hashes = [next(iter(v)) for v in keys.values()]
    assert len(keys) >= 55 and len(set(hashes)) == len(keys)  # pairwise distinct over the distinct shapes


def test_object_hash_is_np_objects_hash_of_the_shape_alone(golhip):
    for name, a in shapes_under_test(golhip).items():
        board = np.zeros((1, 32, 32), dtype=np.uint8)
        board[0, 9:9 + a.shape[0], 20:20 + a.shape[1]] = a
        # reach 2 may still see a random shape as several clusters: place it as ONE object by hand
        ys, xs = np.nonzero(board[0])
        x0, y0 = xs.min(), ys.min()
        want = cases.shape_hash(xs - x0, ys - y0, xs.max() - x0 + 1, ys.max() - y0 + 1)
        assert golhip.object_hash(a) == want, name
        records = cases.np_objects(board, "plane", 2)[0]
        if len(records) == 1:
            assert int(records["hash"][0]) == want and records["population"][0] == a.sum(), name
    names = golhip.common_object_hashes()
    assert sorted(set(names.values())) == sorted(golhip.common_objects()) and len(names) == 10
    for name, arrays in golhip.common_objects().items():  # every phase and orientation of the catalogue
        for a in arrays:
            assert names[golhip.object_hash(a)] == name
    with pytest.raises(golhip.GolHipError):
        golhip.object_hash(np.zeros((3, 3)))
    with pytest.raises(golhip.GolHipError):
        golhip.object_hash(np.ones(3))


# ------------------------------------------------------------------------------ the case table
def test_the_table_is_complete():
    assert len(cases.SHAPES) == 13
    for shape in cases.SHAPES:
        for t in cases.TOPOLOGIES:
            for r in cases.REACHES:
                fams = {f for (w, h, tt, f, rr) in cases.CASES if (w, h) == shape and tt == t and rr == r}
                assert {"sweep", "winds", "soup"} <= fams
                assert ("gap" in fams) == (shape not in cases.ONE_BOARD)
                assert ("cap" in fams) == (shape in cases.CAP_SHAPES)
    for shape in cases.ONE_BOARD:
        for c in cases.CASES:
            if c[:2] == shape:
                assert cases.case(*c)[0].shape[0] == 1
    assert len(set(cases.CASE_IDS)) == len(cases.CASES)
    snakes = [c for c in cases.CASES if c[3] == "snake"]
    assert sorted(snakes) == sorted((64, 64, t, "snake", r) for t in cases.TOPOLOGIES for r in cases.REACHES)


@pytest.mark.parametrize("topology", cases.TOPOLOGIES)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_the_sweep_meets_its_conditions(golhip, shape, topology):
    w, h = shape
    for reach in cases.REACHES:
        boards, meta = cases.case(w, h, topology, "sweep", reach)
        ref = cases.expected(w, h, topology, "sweep", reach)
        obj = meta["obj"]
        oh, ow = obj.shape
        # the plane cuts the object at the border: only its dead corner is left of it at (w - 1, h - 1)
        assert sum(not b.any() for b in boards) <= (2 if topology == "plane" else 0)
        if shape not in cases.ONE_BOARD:
            assert len(boards) == 3 * w + len({0, min(31, w - 1)}) * h  # rows 0, 1, h - 1; columns 0, 31
        steady = 0
        for (x, y), whole, rec in zip(meta["offsets"], meta["whole"], ref):
            if not whole:
                assert topology == "plane" and sum(r["population"] for r in rec) < obj.sum()
                continue
            assert len(rec) == 1 and rec[0]["population"] == obj.sum()
            if not rec[0]["flags"] & (WINDS_X | WINDS_Y):
                steady += 1
                assert int(rec[0]["hash"]) == golhip.object_hash(obj)
                assert (rec[0]["x"], rec[0]["y"], rec[0]["w"], rec[0]["h"]) == (x, y, ow, oh)
            if topology == "plane":
                assert bool(rec[0]["flags"] & AT_BORDER) == (x == 0 or y == 0 or x + ow == w or y + oh == h)
        if w > ow + 2 and h > oh + 2:
            assert steady == sum(meta["whole"])  # nothing winds where there is room
            if topology == "torus" and shape not in cases.ONE_BOARD:  # and the object crosses both seams
                assert ow == 1 or any(x + ow > w for (x, y) in meta["offsets"])
                assert any(y + oh > h for (x, y) in meta["offsets"])
        if shape in cases.ONE_BOARD and topology == "torus":
            assert meta["offsets"][0] == (w - 2, h - 2) and steady == 1


@pytest.mark.parametrize("topology", cases.TOPOLOGIES)
@pytest.mark.parametrize("reach", cases.REACHES)
def test_the_gap_meets_its_conditions(topology, reach):
    """At shapes with room on both axes: one cluster at distance reach, two at reach + 1; on the torus
    also across the seam, on the plane never across the border."""
    seen = {"joined": 0, "apart": 0, "seam-joined": 0, "border-apart": 0, "word-seam": 0}
    for w, h in cases.SHAPES:
        if (w, h) in cases.ONE_BOARD or w < 8 or h < 8:
            continue
        _, meta = cases.case(w, h, topology, "gap", reach)
        ref = cases.expected(w, h, topology, "gap", reach)
        for ((x, y), (x2, y2), d, (sx, sy)), rec in zip(meta["pairs"], ref):
            wrapped = x + sx * d >= w or y + sy * d >= h
            if not wrapped or topology == "torus":
                assert len(rec) == (1 if d == reach else 2), (w, h, x, y, d)
                seen["joined" if d == reach else "apart"] += 1
                seen["seam-joined"] += wrapped and d == reach
                seen["word-seam"] += x == 31 and sx == 1 and w >= 64
            else:
                assert len(rec) == 2 and any(r["flags"] & AT_BORDER for r in rec)
                seen["border-apart"] += 1
    assert seen["joined"] and seen["apart"] and seen["word-seam"]
    assert seen["seam-joined"] if topology == "torus" else seen["border-apart"]


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_the_winds_meet_their_conditions(shape):
    w, h = shape
    for reach in cases.REACHES:
        for topology in cases.TOPOLOGIES:
            _, meta = cases.case(w, h, topology, "winds", reach)
            ref = cases.expected(w, h, topology, "winds", reach)
            if shape in cases.ONE_BOARD:
                big = max(ref[0], key=lambda r: r["population"])
                assert (big["flags"] & (WINDS_X | WINDS_Y)) == (WINDS_X | WINDS_Y if topology == "torus" else 0)
                continue
            by = dict(zip(meta["kinds"], ref))
            if topology == "plane":
                assert not any(r["flags"] & (WINDS_X | WINDS_Y) for rec in ref for r in rec)
                assert (by["row"][0]["x"], by["row"][0]["w"]) == (0, w) and (by["column"][0]["y"], by["column"][0]["h"]) == (0, h)
                continue
            for kind in ("row", "board", "dotted-linked"):
                assert len(by[kind]) == 1 and by[kind][0]["flags"] & WINDS_X, kind
                assert (by[kind][0]["x"], by[kind][0]["w"]) == (0, w), kind
            assert len(by["column"]) == 1 and by["column"][0]["flags"] & WINDS_Y
            assert (by["column"][0]["y"], by["column"][0]["h"]) == (0, h)
            assert by["board"][0]["flags"] & WINDS_Y and by["board"][0]["population"] == w * h
            if w >= 8:  # the dotted row with gaps of reach falls apart where the row has room for two gaps
                assert len(by["dotted-apart"]) > 1
                assert bool(by["row"][0]["flags"] & WINDS_Y) == (h <= reach)


def test_the_snake_and_the_cap_meet_their_conditions():
    for topology in cases.TOPOLOGIES:
        for reach in cases.REACHES:
            boards, meta = cases.case(64, 64, topology, "snake", reach)
            ref = cases.expected(64, 64, topology, "snake", reach)
            for kind, b, rec in zip(meta["kinds"], boards, ref):
                cut = kind.endswith("cut")
                assert len(rec) == (2 if cut and reach == 1 else 1), (kind, reach)
                assert sum(r["population"] for r in rec) == b.sum() > 58 * 58 // (reach + 1)
            assert int(ref[0][0]["hash"]) == int(ref[1][0]["hash"])  # the transpose is an orientation
            for w, h in cases.CAP_SHAPES:
                _, meta = cases.case(w, h, topology, "cap", reach)
                rec = cases.expected(w, h, topology, "cap", reach)[0]
                assert len(rec) == meta["clusters"] > max(cases.CAP_LIMITS) and (rec["population"] == 1).all()
                assert len(set(rec["hash"].tolist())) == 1
                order = rec["y"].astype(np.int64) * w + rec["x"]
                assert (np.diff(order) > 0).all()  # row-major


def test_the_soups_hold_many_clusters_of_more_than_one_cell():
    for c in cases.CASES:
        if c[3] != "soup" or c[0] * c[1] < 256:
            continue
        ref = cases.expected(*c)
        assert max(len(r) for r in ref) >= 2 and max(r["population"].max() for r in ref if len(r)) >= 3, c
    # the cap is reached: a 512 x 128 soup at reach 1 has more than 4096 clusters
    assert max(len(r) for r in cases.expected(512, 128, "torus", "soup", 1)) > 4096
