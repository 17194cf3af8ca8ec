"""Batch.objects and Batch.search_objects (golhip_batch_objects, golhip_batch_search_objects: gol_batch_objects,
csrc/batch_objects.hpp) against np_objects of tests/objects_cases.py, the reference written from the
definitions of include/golhip.h.  Every comparison is exact: the number of clusters, their order, x,
y, w, h, population, flags and the 64-bit hash.

The case table (13 shapes x 2 topologies x families x both reaches) and the reference live in
tests/objects_cases.py; tests/test_batch_objects_cpu.py shows without a GPU that the table is complete
and that the reference meets each family's conditions.  Here the kernel is held to the reference, and
the families' conditions are asserted on the kernel's own records where they say more than equality
with the reference does."""
import os
import subprocess
import sys

import numpy as np
import pytest

import objects_cases as cases
from conftest import PKG
from objects_cases import AT_BORDER, CAP_LIMITS, CAP_SHAPES, REACHES, TOPOLOGIES, WINDS_X, WINDS_Y

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def run_objects(golhip, boards, topology, reach, max_objects):
    n, h, w = boards.shape
    with golhip.Batch(w, h, n, topology=topology) as b:
        b.load(boards * 255)
        return b.objects(max_objects=max_objects, reach=reach)


def assert_equal_tables(got, want, what):
    (gn, go), (wn, wo) = got, want
    assert gn.dtype == np.int32 and go.dtype == cases.OBJECT_DTYPE and go.shape == wo.shape
    assert np.array_equal(gn, wn), (what, np.nonzero(gn != wn)[0][:8], gn[gn != wn][:8], wn[gn != wn][:8])
    bad = np.argwhere(go != wo)
    assert len(bad) == 0, (what, bad[:4], [(go[tuple(i)], wo[tuple(i)]) for i in bad[:4]])


# ---------------------------------------------------------------- 1. every case against the reference
@pytest.mark.parametrize("width,height,topology,family,reach", cases.CASES, ids=cases.CASE_IDS)
def test_1_objects_are_np_objects(golhip, width, height, topology, family, reach):
    boards, meta = cases.case(width, height, topology, family, reach)
    ref = cases.expected(width, height, topology, family, reach)
    most = max(len(r) for r in ref)
    max_objects = min(max(most, 1), golhip.OBJECTS_MAX)
    got = run_objects(golhip, boards, topology, reach, max_objects)
    assert_equal_tables(got, cases.table(ref, max_objects), (width, height, topology, family, reach))
    n, o = got
    if family == "sweep":
        # one hash wherever the whole object lies without winding; the extent follows it across the seam
        ow, oh = meta["obj"].shape[1], meta["obj"].shape[0]
        key = golhip.object_hash(meta["obj"])
        for i, ((x, y), whole) in enumerate(zip(meta["offsets"], meta["whole"])):
            rec = o[i, 0]
            if whole and n[i] == 1 and not rec["flags"] & (WINDS_X | WINDS_Y):
                assert int(rec["hash"]) == key and (rec["x"], rec["y"], rec["w"], rec["h"]) == (x, y, ow, oh), (i, rec)
            if topology == "plane" and whole:
                edge = x == 0 or y == 0 or x + ow == width or y + oh == height
                assert bool(rec["flags"] & AT_BORDER) == edge, (i, rec)
    if family == "cap":
        assert n[0] == meta["clusters"] > max(CAP_LIMITS)


# ---------------------------------------------------------------- 2. the cap only cuts the list
@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("topology", TOPOLOGIES)
@pytest.mark.parametrize("shape", CAP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_2_the_cap_cuts_the_list_and_leaves_the_rest_alone(golhip, shape, topology, reach):
    w, h = shape
    boards, meta = cases.case(w, h, topology, "cap", reach)
    ref = cases.expected(w, h, topology, "cap", reach)
    lib = golhip.load_library()
    with golhip.Batch(w, h, 1, topology=topology) as b:
        b.load(boards * 255)
        for cap in CAP_LIMITS:
            n = np.full(1, -7, dtype=np.int32)
            o = np.full((1, cap + 3), SENTINEL, dtype=np.uint8).repeat(32, axis=1).view(cases.OBJECT_DTYPE)
            guard = o.copy()
            assert lib.golhip_batch_objects(b._h, cap, reach, n.ctypes.data, o.ctypes.data) == 0
            assert n[0] == meta["clusters"] == len(ref[0])
            assert np.array_equal(o[0, :cap], ref[0][:cap])
            assert np.array_equal(o[0, cap:], guard[0, cap:])  # the sentinel behind the records
            assert b.objects(max_objects=cap, reach=reach)[0][0] == n[0]
        counts = np.zeros(1, dtype=np.int32)  # the counts alone
        assert lib.golhip_batch_objects(b._h, 1, reach, counts.ctypes.data, None) == 0 and counts[0] == meta["clusters"]


CHILD = """
import sys
sys.path.insert(0, {pkg!r})
import numpy as np
import golhip
boards = np.load({inp!r})
with golhip.Batch(boards.shape[2], boards.shape[1], boards.shape[0], topology={topology!r}) as b:
    b.load(boards)
    n, o = b.objects(max_objects={cap}, reach={reach})
    np.savez({out!r}, n=n, o=o)
"""


@pytest.mark.parametrize("reach", REACHES)
def test_2_the_result_does_not_depend_on_the_stage(golhip, tmp_path, reach):
    """A fresh process whose stage is 100 bytes (GOLHIP_STAGE_BYTES): a count and three records, so a
    board at a time and max_objects 7 in three launches: the grid of the cap family and 12 soups of
    16 x 64."""
    cap = 7
    grid, _ = cases.case(16, 64, "torus", "cap", reach)
    soup, _ = cases.case(16, 64, "torus", "soup", reach)
    boards = np.concatenate([grid, soup])
    want = run_objects(golhip, boards, "torus", reach, cap)
    assert_equal_tables(want, cases.table(cases.np_objects(boards, "torus", reach), cap), "in process")
    np.save(tmp_path / "in.npy", boards * 255)
    code = CHILD.format(pkg=str(PKG), inp=str(tmp_path / "in.npy"), out=str(tmp_path / "out.npz"), topology="torus",
                        cap=cap, reach=reach)
    env = dict(os.environ, GOLHIP_STAGE_BYTES="100")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, "-c", code], env=env, check=True, timeout=120)
    small = np.load(tmp_path / "out.npz")
    assert_equal_tables((small["n"], small["o"]), want, "stage of 100 bytes")


# ---------------------------------------------------------------- 3. ash the device stepped
@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("topology", TOPOLOGIES)
@pytest.mark.parametrize("shape", [(16, 64), (64, 64), (128, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_3_the_ash_of_soups_at_turn_200(golhip, shape, topology, reach):
    w, h = shape
    n = 24
    rng = np.random.default_rng([w, h, 200])
    soups = (rng.random((n, h, w)) < 0.5).astype(np.uint8)
    with golhip.Batch(w, h, n, topology=topology) as b:
        b.load(soups * 255)
        b.step(200)
        before = b.store()
        nobj, obj = b.objects(max_objects=64, reach=reach)
        assert b.turn == 200 and np.array_equal(b.store(), before)  # the boards and the turn stay
        again = b.objects(max_objects=64, reach=reach)
        assert np.array_equal(again[0], nobj) and np.array_equal(again[1], obj)
    ash = (before != 0).astype(np.uint8)
    assert ash.any()
    assert_equal_tables((nobj, obj), cases.table(cases.np_objects(ash, topology, reach), 64), (shape, topology, reach))


# ---------------------------------------------------------------- 4. the search
SEARCH = [((64, 64), list(range(100, 112)), 4000), ((128, 16), list(range(7, 19)), 3000)]
TOO_SHORT = 60  # generations within which hardly a 64 x 64 soup repeats


@pytest.mark.parametrize("topology", TOPOLOGIES)
@pytest.mark.parametrize("shape,seeds,max_turns", SEARCH, ids=["64x64", "128x16"])
def test_4_search_objects_is_objects_of_the_recipe_board(golhip, shape, seeds, max_turns, topology):
    w, h = shape
    seeds = np.array(seeds, dtype=np.uint64)
    pats = [p for ps in golhip.common_objects().values() for p in ps if p.shape[0] <= h]
    with golhip.Batch(w, h, 1, topology=topology) as b:
        got = b.search_objects(len(seeds), seeds=seeds, max_turns=max_turns)
        census = b.search_census(len(seeds), pats, seeds=seeds, max_turns=max_turns)
        one = b.search_objects(len(seeds), seeds=seeds, max_turns=max_turns, reach=1, max_objects=5)
        # the result does not depend on how nsoups is cut
        parts = [b.search_objects(len(s), seeds=s, max_turns=max_turns) for s in (seeds[:5], seeds[5:6], seeds[6:])]
        short = b.search_objects(len(seeds), seeds=seeds, max_turns=TOO_SHORT if h == 64 else 4)
    assert got.records.tobytes() == census.records.tobytes()
    assert np.array_equal(got.cycle_start, census.cycle_start) and np.array_equal(got.ash_turn, census.ash_turn)
    assert np.array_equal(one.ash_turn, census.ash_turn) and one.records.tobytes() == census.records.tobytes()
    for k, field in enumerate(got._fields):
        joined = np.concatenate([p[k] for p in parts])
        assert joined.tobytes() == got[k].tobytes(), field
    repeated = got.records["repeat_turn"] >= 0
    assert 2 * int(repeated.sum()) >= len(seeds) and got.nobjects.any()
    for i, seed in enumerate(seeds):
        if not repeated[i]:
            assert got.ash_turn[i] == -1 and got.nobjects[i] == 0 and one.nobjects[i] == 0
            continue
        with golhip.Batch(w, h, 1, topology=topology) as r:
            r.init_random(seeds=[seed])
            r.step(int(got.ash_turn[i]))
            for res, reach, cap in ((got, 2, 64), (one, 1, 5)):
                n, o = r.objects(max_objects=cap, reach=reach)
                assert n[0] == res.nobjects[i] and np.array_equal(o[0], res.objects[i]), (i, reach)
    # a soup without a repeat: ash_turn -1, no cluster, no record
    lost = short.records["repeat_turn"] < 0
    assert lost.any()
    assert (short.ash_turn[lost] == -1).all() and not short.nobjects[lost].any()
    assert not short.objects[lost].view(np.uint8).any()


# ---------------------------------------------------------------- 5. errors
def test_5_refused_calls_touch_nothing(golhip):
    lib = golhip.load_library()
    boards = np.zeros((3, 8, 64), dtype=np.uint8)
    boards[:, 2, 3] = 255
    with golhip.Batch(64, 8, 3) as b:
        b.load(boards)
        b.step(1)
        n = np.full(3, -7, dtype=np.int32)
        o = np.full((3, 4 * 32), SENTINEL, dtype=np.uint8)
        for max_objects, reach, nptr in ((0, 2, n.ctypes.data), (4097, 2, n.ctypes.data), (4, 0, n.ctypes.data),
                                         (4, 3, n.ctypes.data), (4, 2, None)):
            rc = lib.golhip_batch_objects(b._h, max_objects, reach, nptr, o.ctypes.data)
            assert rc == golhip.ERR_ARG, (max_objects, reach, rc)
            assert b"objects" in lib.golhip_batch_last_error(b._h)
            assert (n == -7).all() and (o == SENTINEL).all() and b.turn == 1
        for kw in (dict(max_objects=0), dict(max_objects=4097), dict(reach=0), dict(reach=3)):
            with pytest.raises(golhip.GolHipError) as e:
                b.objects(**kw)
            assert e.value.code == golhip.ERR_ARG
            with pytest.raises(golhip.GolHipError) as e:
                b.search_objects(2, max_turns=10, **kw)
            assert e.value.code == golhip.ERR_ARG
        # the search's outputs stay too
        out = np.full(2 * 32, SENTINEL, dtype=np.uint8)
        i64 = [np.full(2, -7, dtype=np.int64) for _ in range(2)]
        no = np.full(2, -7, dtype=np.int32)
        for max_objects, reach, noptr in ((0, 2, no.ctypes.data), (4, 3, no.ctypes.data), (4, 2, None)):
            rc = lib.golhip_batch_search_objects(b._h, 2, None, 1, golhip.DENSITY_HALF, 10, None, None, max_objects, reach,
                                                 out.ctypes.data, i64[0].ctypes.data, i64[1].ctypes.data, noptr,
                                                 o.ctypes.data)
            assert rc == golhip.ERR_ARG
            assert (out == SENTINEL).all() and all((a == -7).all() for a in i64) and (no == -7).all()
            assert (o == SENTINEL).all()
        # and the batch still works
        nobj, obj = b.objects(max_objects=4)
        assert (nobj == 0).all() and b.turn == 1  # a lone cell dies
