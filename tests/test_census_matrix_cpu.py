"""The case table of the census matrix (tests/census_matrix_cases.py) without a GPU: np_census, the
vectorised reference, agrees exactly with ref_census, the brute force of tests/test_gpu_batch_census.py,
on that module's own cases and on 400 small random (board, pattern, topology) triples; the table has
every shape x topology x family that fits, within its limits, and every pattern passes
golhip.pattern(); and no case is vacuous.  The conditions are on np_census's results alone.

The expected values of the whole table (130 cases, test_the_table_is_within_its_limits computes all
of them and prints the time) take np_census 7 seconds on one CPU core (measured: 6.4 s), most of it the 32 x 32
patterns of the skipped-row cases at 64 x 512 and 512 x 128 on the plane; no case takes a second."""
import time

import numpy as np
import pytest

import census_matrix_cases as T
import test_gpu_batch_census as C
from census_matrix_cases import np_census


def cases_of(family):
    return [c for c in T.CASES if c[3] == family]


def ids_of(family):
    return [f"{w}x{h}-{t}" for w, h, t, _ in cases_of(family)]


# ---------------------------------------------------------------- np_census is ref_census
def test_np_census_on_the_existing_cases(golhip, monkeypatch):
    """Tests 1 to 6 of tests/test_gpu_batch_census.py, the 512 x 512 boards of test 5 included, with their
    check() replaced: what they would ask of the device they ask of np_census and ref_census, which
    must agree; their own assertions then run on that result.  Test 7's board is rebuilt here."""
    seen = []

    def both(golhip, boards, patterns, topology):
        boards = np.asarray(boards, dtype=np.uint8)
        rc, rr = C.ref_all(boards, patterns, topology)
        nc, nr = np_census(boards, patterns, topology)
        assert np.array_equal(nc, rc) and np.array_equal(nr, rr), (topology, nc.tolist(), rc.tolist(), nr, rr)
        seen.append((boards.shape, len(patterns), topology))
        return nc, nr

    monkeypatch.setattr(C, "check", both)
    C.test_1_a_block_a_block_over_the_corner_and_nothing(golhip)
    C.test_2_the_borders_of_a_plane(golhip)
    C.test_3_word_seams(golhip)
    for topology in T.TOPOLOGIES:
        C.test_4_rows_narrower_than_a_word(golhip, topology)
        C.test_5_the_largest_frame(golhip, topology)
    C.test_6_overlaps_and_cells_not_looked_at(golhip)
    b = np.zeros((1, 32, 64), dtype=np.uint8)
    C.put(b[0], C.BLOCK, 4, 4)
    C.put(b[0], C.RPENT, 40, 20)
    counts, residue = both(golhip, b, [golhip.isolated(C.BLOCK)], "torus")
    assert counts[0, 0] == 1 and residue[0] == 5
    assert len(seen) == 18 and ((1, 512, 512), 33, "plane") in seen


def test_np_census_on_random_triples():
    """400 triples: boards of 1 to 12 cells a side (any size, not only the engine's) at a random
    density, 1 to 4 patterns of any size that fits with any share of their cells not looked at; and
    8 with boards of 33 to 40 cells and patterns up to 32 x 32 cut from them."""
    rng = np.random.default_rng(2024)
    matches = 0
    for i in range(408):
        small = i < 400
        H, W = (int(v) for v in (rng.integers(1, 13, 2) if small else rng.integers(33, 41, 2)))
        boards = (rng.random((2, H, W)) < rng.random()).astype(np.uint8)
        pats = []
        while len(pats) < rng.integers(1, 5):
            h, w = int(rng.integers(1, min(H, 32) + 1)), int(rng.integers(1, min(W, 32) + 1))
            if small and rng.random() < 0.5:
                p = (rng.random((h, w)) < rng.random()).astype(np.int8)
            else:  # cut from board 0, wrapped: it matches there on the torus
                y, x = int(rng.integers(H)), int(rng.integers(W))
                p = boards[0][np.ix_((y + np.arange(h)) % H, (x + np.arange(w)) % W)].astype(np.int8)
            p[rng.random((h, w)) < rng.random() * 0.8] = -1
            if (p == 1).any():
                pats.append(p)
        topology = T.TOPOLOGIES[i % 2]
        rc, rr = C.ref_all(boards, pats, topology)
        nc, nr = np_census(boards, pats, topology)
        assert np.array_equal(nc, rc) and np.array_equal(nr, rr), (i, topology, boards.tolist(), [p.tolist() for p in pats])
        matches += int(rc.sum())
    assert matches > 1000


# ---------------------------------------------------------------- the table is complete
def test_the_table_has_every_shape_topology_and_family():
    for must in [(1, 4), (2, 8), (8, 16), (16, 64), (32, 4), (32, 32), (64, 512), (128, 8), (256, 32), (512, 4),
                 (512, 128), (512, 512)]:
        assert must in T.SHAPES
    assert {w for w, _ in T.SHAPES} == {1, 2, 4, 8, 16, 32, 64, 128, 256, 512}  # every width the engine makes
    assert {h for _, h in T.SHAPES} == {4, 8, 16, 32, 64, 128, 256, 512}        # every height
    for shape in T.SHAPES:
        fits = {f for f in T.FAMILIES if f != "selfwrap" or 2 <= shape[0] <= 16}
        if shape in T.ONE_BOARD:
            assert shape == (512, 512) and set(T.families_of(shape)) == {"largest"}, T.ONE_BOARD[shape]
        else:
            assert set(T.families_of(shape)) == fits, shape
        for topology in T.TOPOLOGIES:
            for family in T.families_of(shape):
                assert (*shape, topology, family) in T.CASES
    assert len(T.CASES) == len(set(T.CASES)) == 2 * (12 * 5 + 4 + 1)
    # the workgroups: 64 lanes (up to 64 items) and 1024 that loop (more than 1024 items), and item
    # counts that are no multiple of 64: a lane per 32 anchors of a row, a plane has 31 more rows and
    # a word more per row
    items = {(w, h, t): (h + 31) * (max(w // 32, 1) + 1) if t == "plane" else h * max(w // 32, 1)
             for w, h in T.SHAPES for t in T.TOPOLOGIES}
    assert sum(n <= 64 for n in items.values()) >= 6 and sum(n > 1024 for n in items.values()) >= 4
    assert sum(n % 64 != 0 for n in items.values()) >= 12
    assert sum(n > 1024 and n % 1024 != 0 for n in items.values()) >= 3


@pytest.mark.parametrize("case", T.CASES, ids=T.CASE_IDS)
def test_every_pattern_is_a_pattern(golhip, case):
    w, h, topology, family = case
    boards, patterns, _ = T.case(*case)
    assert boards.dtype == np.uint8 and boards.max() <= 1 and not boards.flags.writeable
    assert 1 <= boards.shape[0] <= 96 and 1 <= len(patterns) <= 24
    for p in patterns:
        q = golhip.pattern(p)  # raises for what golhip_batch_census refuses in a pattern
        assert q.w <= w and q.h <= h and (q.h, q.w) == p.shape and not p.flags.writeable


def test_the_table_is_within_its_limits():
    """Every expected value, computed here once (the tests below and the GPU module read the cache),
    and the time it took."""
    t0, worst = time.perf_counter(), (0.0, None)
    for case in T.CASES:
        t1 = time.perf_counter()
        counts, residue = T.expected(*case)
        worst = max(worst, (time.perf_counter() - t1, case))
        boards, patterns, _ = T.case(*case)
        assert counts.shape == (boards.shape[0], len(patterns)) and residue.shape == (boards.shape[0],)
        assert not counts.flags.writeable and not residue.flags.writeable
        assert (residue <= boards.sum(axis=(1, 2))).all()
    total = time.perf_counter() - t0
    print(f"np_census over the table: {total:.1f} s, the slowest case {worst[1]} {worst[0]:.2f} s")
    assert total < 120  # on the order of a minute at the most


# ---------------------------------------------------------------- no case is vacuous
@pytest.mark.parametrize("case", cases_of("sweep"), ids=ids_of("sweep"))
def test_sweep(case):
    w, h, topology, _ = case
    shape = (w, h)
    boards, patterns, meta = T.case(*case)
    counts, residue = T.expected(*case)
    n = boards.shape[0]
    pop = boards.sum(axis=(1, 2))
    assert (shape in T.NO_RPENTOMINO) == (w < 5 or h < 5) and (shape in T.NO_RING) == (w < 3)
    xs = {x for x, _ in meta["offsets"]}
    assert {x % w for x in range(w - 35, w - 35 + min(w, 70))} <= xs
    assert {y % h for y in range(h - 3, h + 3)} <= {y for _, y in meta["offsets"]}
    if w >= 70:  # every bit of a word, a word seam and the board's seam
        assert {x % 32 for x in xs if x >= 0} == set(range(32)) and {w - 1, 0, w - 32, w - 33} <= xs
    assert len({b.tobytes() for b in boards}) >= min(n, 3)  # the boards of a launch differ
    rows = np.arange(n)
    if shape in T.NO_RING:
        # no ring fits (T.NO_RING[shape]): the condition is on the bare object
        own = counts[rows, meta["bare"]]
    else:
        own = counts[rows, meta["ringed"]]
    if topology == "torus":
        assert (own == 1).all() and (residue == 0).all() and (pop > 0).all(), (shape, own.tolist(), residue.tolist())
        return
    assert (own == 1).any() and (own == 0).any(), (shape, own.tolist())
    assert all(x < 0 or y < 0 for x, y in meta["offsets"][-5:])  # across the left and top border too
    if shape in T.NO_RPENTOMINO:
        # no board has residue > 0 here (the reason stands at T.NO_RPENTOMINO).  The condition is the
        # object's: some board holds less than the object, and its ring does not match
        assert (residue == 0).all(), shape
        assert ((own == 0) & (pop < pop.max())).any(), shape
    else:
        assert ((own == 0) & (residue > 0)).any(), (shape, own.tolist(), residue.tolist())
        assert ((pop > 0) & (pop < 5)).any()  # an object cut at the border


@pytest.mark.parametrize("case", cases_of("largest") + cases_of("skipped"), ids=ids_of("largest") + ids_of("skipped"))
def test_largest_and_skipped(case):
    w, h, topology, family = case
    shape = (w, h)
    boards, patterns, meta = T.case(*case)
    counts, _ = T.expected(*case)
    pw, ph = min(32, w), min(32, h)
    big = [k for k, p in enumerate(patterns) if p.shape == (ph, pw)]
    assert len(big) >= 3 and (family == "skipped" or big[:3] == [0, 1, 2])
    for k, owner in enumerate(meta["owner"]):
        assert counts[owner, k] >= 1, (shape, k)
        others = np.delete(counts[:, k], owner)
        if k not in big:  # a row, a column, the two columns: small enough to match any soup
            continue
        if shape in T.ONE_BOARD:
            assert others.size == 0, T.ONE_BOARD[shape]
        else:
            assert (others == 0).any(), (shape, k, counts[:, k].tolist())
    if family == "largest":
        shapes = [p.shape for p in patterns]
        assert (1, pw) in shapes and (ph, 1) in shapes
        if shape[0] * shape[1] >= 256:  # a third of the cells not looked at
            for k in big:
                assert 0.2 < (patterns[k] < 0).mean() < 0.45
        if w >= 32:
            # shifts by 0 and by 31: cells looked at in columns 0 and 31, of the big ones and of the
            # pattern that looks at nothing else
            for k in big:
                assert (patterns[k][:, 0] >= 0).any() and (patterns[k][:, 31] >= 0).any()
            edge = [p for p in patterns if p.shape[1] == 32 and (p[:, 1:31] < 0).all()]
            assert len(edge) == 1 and (edge[0][:, 0] >= 0).all() and (edge[0][:, 31] >= 0).all()
            assert counts[:, len(patterns) - 1].max() > (1 if w * h >= 1024 else 0)
        anchors = T.largest_anchors(shape, topology)
        if w >= 64:
            assert anchors[0][0] % 32 == 0 and anchors[1][0] % 32 == 31
        if topology == "torus":
            assert (anchors[2][0] + pw > w or w == 1) and anchors[2][1] + ph > h  # across both seams
        else:
            assert anchors[2] == (w - pw, h - ph)
    else:
        assert len(patterns) >= 9 if ph > 4 else len(patterns) >= 6
        for p, rows in zip(patterns, meta["rows"]):
            assert p.shape == (ph, pw) and (p[list(rows)] == -1).all() and (p == 1).any()
        kinds = {rows for rows in meta["rows"]}
        assert {(0,), (ph // 2 - 1, ph // 2), (ph - 1,)} <= kinds
        assert ((0, ph // 2 - 1, ph // 2, ph - 1) in kinds) == (ph > 4)  # of 4 rows none would be left


@pytest.mark.parametrize("case", cases_of("dense"), ids=ids_of("dense"))
def test_dense(case):
    w, h, topology, _ = case
    shape = (w, h)
    boards, patterns, _ = T.case(*case)
    counts, residue = T.expected(*case)
    pop = boards.sum(axis=(1, 2))
    assert len(patterns) == 18 - (w < 2)
    for p in patterns[:16]:
        assert p.shape == (3, min(3, w)) and min(3, p.size) <= (p >= 0).sum() <= 6 and (p == 1).any()
    assert [(p == 1).all() for p in patterns[16:]] == [True] * (len(patterns) - 16)
    if w >= 2:  # 3, 4, 5 and 6 cells looked at all occur
        assert {int((p >= 0).sum()) for p in patterns[:16]} == {3, 4, 5, 6}
    density = pop / (w * h)
    assert (density > 0.8).any() and (density < 0.3).any()
    if shape in T.FEW_ANCHORS:
        assert w * h <= 32 and counts.max() >= 2, T.FEW_ANCHORS[shape]
    else:
        assert counts.max() > 32, shape  # more than one lane's anchors
        assert (counts.max(axis=0) > 0).sum() >= 12  # and most patterns match somewhere
    if shape in T.ALL_EXPLAINED:
        assert w == 1 and (residue == 0).all(), T.ALL_EXPLAINED[shape]
    else:
        assert ((residue > 0) & (residue < pop)).any(), (shape, residue.tolist())


@pytest.mark.parametrize("case", cases_of("selfwrap"), ids=ids_of("selfwrap"))
def test_selfwrap(case):
    w, h, topology, _ = case
    boards, patterns, meta = T.case(*case)
    counts, residue = T.expected(*case)
    assert all(p.shape[1] == w for p in patterns) and 2 <= w <= 16
    full, row = meta["full_row"], meta["row"]
    assert boards[full].sum() == w and patterns[row].shape == (1, w) and (patterns[row] == 1).all()
    assert counts[full, row] == (w if topology == "torus" else 1) and residue[full] == 0
    assert counts[7, row] == (w * h if topology == "torus" else h)  # the board all alive
    cut = counts[:3, :row]
    if topology == "torus":  # every cut matches the soup it was cut from, wrapped onto itself
        assert all(cut[j, 2 * j] >= 1 and cut[j, 2 * j + 1] >= 1 for j in range(3)) and row == 6
    else:
        assert cut[0, 0] >= 1
    assert ((residue > 0) & (residue < boards.sum(axis=(1, 2)))).any()


@pytest.mark.parametrize("case", cases_of("mixed"), ids=ids_of("mixed"))
def test_mixed(case):
    w, h, topology, _ = case
    boards, patterns, meta = T.case(*case)
    counts, residue = T.expected(*case)
    kinds = meta["kinds"]
    assert len(kinds) == len(patterns) and kinds[:3] == ["N", "R", "E"] and set(kinds) == {"N", "R", "E"}
    total = counts.sum(axis=0)
    assert (total == 0).any() and (counts > 0).all(axis=0).any()
    if w >= 32:
        # from 32 columns on: no N pattern matches, every E pattern matches on every board, the R
        # patterns once per board (a wrapped cut does not match on the plane)
        for k, kind in enumerate(kinds):
            if kind == "N":
                assert total[k] == 0, k
            elif kind == "E":
                assert (counts[:, k] > (32 if w * h >= 1024 else 0)).all(), k
            elif topology == "torus" or k == kinds.index("R"):
                assert (counts[:, k] == 1).all(), (k, counts[:, k].tolist())
        assert kinds.count("R") == 3 and 0 < meta["row"] < h - 1
    pop = boards.sum(axis=(1, 2))
    if (w, h) in T.MOSTLY_SIGNATURE:
        assert w * h < 256, T.MOSTLY_SIGNATURE[(w, h)]
    else:
        assert ((residue > 0) & (residue < pop)).all(), (w, h)
    # the reversed list: the same columns the other way round, the same residue
    rc, rr = np_census(boards, patterns[::-1], topology)
    assert np.array_equal(rc, counts[:, ::-1]) and np.array_equal(rr, residue)
