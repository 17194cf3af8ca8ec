"""golhip.Batch.census on the GPU: per board, how often each pattern matches and how many live cells no
match covers, against a numpy brute force written here from the definitions in include/golhip.h.
Every comparison is exact integer equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ the reference
def ref_census(board, patterns, topology):
    """(counts, residue) of one board (h, w; nonzero = alive) from the definitions.  A plane is
    padded with 31 dead cells on every side, so that every anchor -(w - 1) .. width - 1 is an
    ordinary position; a torus is tiled far enough for a pattern to wrap and matched at the anchors
    of the first tile only.  Patterns are arrays of 1 / 0 / -1."""
    a = (np.asarray(board) != 0)
    H, W = a.shape
    counts = np.zeros(len(patterns), dtype=np.int64)
    covered = np.zeros((H, W), dtype=bool)
    if topology == "plane":
        big = np.pad(a, 31)
    else:
        big = np.tile(a, (1 + -(-31 // H), 1 + -(-31 // W)))
    for k, p in enumerate(patterns):
        p = np.asarray(p)
        h, w = p.shape
        if topology == "plane":
            ny, nx = H + h - 1, W + w - 1          # anchors -(h - 1) .. H - 1 and -(w - 1) .. W - 1
            oy, ox = 31 - (h - 1), 31 - (w - 1)    # where anchor (-(w - 1), -(h - 1)) lies in `big`
        else:
            ny, nx, oy, ox = H, W, 0, 0
        m = np.ones((ny, nx), dtype=bool)
        for r in range(h):
            for c in range(w):
                if p[r, c] < 0:
                    continue
                m &= big[oy + r:oy + r + ny, ox + c:ox + c + nx] == (p[r, c] == 1)
        counts[k] = m.sum()
        for y, x in zip(*np.nonzero(m)):
            for r, c in zip(*np.nonzero(p == 1)):
                if topology == "plane":
                    yy, xx = y + oy - 31 + r, x + ox - 31 + c
                    assert 0 <= yy < H and 0 <= xx < W  # a live cell of a match lies on the board
                else:
                    yy, xx = (y + r) % H, (x + c) % W
                covered[yy, xx] = True
    return counts, int((a & ~covered).sum())


def ref_all(boards, patterns, topology):
    res = [ref_census(b, patterns, topology) for b in boards]
    return np.array([r[0] for r in res]).reshape(len(boards), len(patterns)), np.array([r[1] for r in res])


def check(golhip, boards, patterns, topology):
    boards = np.asarray(boards, dtype=np.uint8)
    n, hh, ww = boards.shape
    with golhip.Batch(ww, hh, n, topology=topology) as b:
        b.load(boards)
        counts, residue = b.census(patterns)
        alive = b.alive_counts()
    assert counts.dtype == np.uint32 and counts.shape == (n, len(patterns))
    assert residue.dtype == np.uint32 and residue.shape == (n,)
    rc, rr = ref_all(boards, patterns, topology)
    assert np.array_equal(counts, rc), (topology, counts.tolist(), rc.tolist())
    assert np.array_equal(residue, rr), (topology, residue.tolist(), rr.tolist())
    assert np.array_equal(alive, (boards != 0).sum(axis=(1, 2)))
    return counts, residue


def put(board, cells, x, y):
    """cells (1 = alive) with its top-left corner at (x, y), wrapped."""
    cells = np.asarray(cells)
    H, W = board.shape
    for r, c in zip(*np.nonzero(cells == 1)):
        board[(y + r) % H, (x + c) % W] = 255


BLOCK = np.ones((2, 2), dtype=np.int8)
BLINKER = np.ones((1, 3), dtype=np.int8)
BEEHIVE = np.array([[0, 1, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0]], dtype=np.int8)
RPENT = np.array([[0, 1, 1], [1, 1, 0], [0, 1, 0]], dtype=np.int8)


# ---------------------------------------------------------------------------------- the cases
def test_1_a_block_a_block_over_the_corner_and_nothing(golhip):
    boards = np.zeros((3, 16, 16), dtype=np.uint8)
    put(boards[0], BLOCK, 3, 3)
    put(boards[1], BLOCK, 15, 15)
    assert boards[1][15, 15] and boards[1][15, 0] and boards[1][0, 15] and boards[1][0, 0]
    iso = golhip.isolated(BLOCK)
    counts, residue = check(golhip, boards, [iso], "torus")
    assert counts[:, 0].tolist() == [1, 1, 0] and residue.tolist() == [0, 0, 0]
    counts, residue = check(golhip, boards, [iso], "plane")
    assert counts[:, 0].tolist() == [1, 0, 0] and residue.tolist() == [0, 4, 0]


def test_2_the_borders_of_a_plane(golhip):
    """A block in each corner, a blinker along each edge: the rings lie outside, the anchors are
    negative, every object counts."""
    b = np.zeros((16, 16), dtype=np.uint8)
    for x, y in ((0, 0), (14, 0), (0, 14), (14, 14)):
        put(b, BLOCK, x, y)
    put(b, BLINKER, 6, 0)
    put(b, BLINKER, 6, 15)
    put(b, BLINKER.T, 0, 6)
    put(b, BLINKER.T, 15, 6)
    pats = [golhip.isolated(BLOCK), golhip.isolated(BLINKER), golhip.isolated(BLINKER.T)]
    counts, residue = check(golhip, [b], pats, "plane")
    assert counts[0].tolist() == [4, 2, 2] and residue[0] == 0


def test_3_word_seams(golhip):
    b = np.zeros((8, 128), dtype=np.uint8)
    put(b, BEEHIVE, 30, 1)
    put(b, BEEHIVE, 62, 4)
    pats = [golhip.isolated(o) for o in golhip.orientations(BEEHIVE)]
    counts, residue = check(golhip, [b], pats, "plane")
    assert counts[0].tolist() == [2, 0] and residue[0] == 0
    put(b, BEEHIVE, 126, 1)  # columns 126, 127, 0, 1
    counts, residue = check(golhip, [b], pats, "torus")
    assert counts[0].tolist() == [3, 0] and residue[0] == 0
    counts, residue = check(golhip, [b], pats, "plane")  # cut in two on a plane: 6 cells left over
    assert counts[0].tolist() == [2, 0] and residue[0] == 6


@pytest.mark.parametrize("topology", ["torus", "plane"])
def test_4_rows_narrower_than_a_word(golhip, topology):
    """16 and 4 cells wide: a word holds 2 and 8 replicas of the row; an object counts once."""
    b = np.zeros((2, 16, 16), dtype=np.uint8)
    put(b[0], BLINKER, 5, 7)
    put(b[1], BLOCK, 13, 2)
    pats = [golhip.isolated(BLINKER), golhip.isolated(BLOCK), golhip.isolated(BLINKER.T)]
    counts, residue = check(golhip, b, pats, topology)
    assert counts.tolist() == [[1, 0, 0], [0, 1, 0]] and residue.tolist() == [0, 0]
    s = np.zeros((2, 4, 4), dtype=np.uint8)
    put(s[0], BLOCK, 1, 1)
    put(s[1], BLOCK, 3, 3)  # over the corner
    counts, residue = check(golhip, s, [golhip.isolated(BLOCK), BLOCK], topology)
    if topology == "torus":  # the 4 x 4 pattern on the 4 x 4 torus: one anchor each
        assert counts.tolist() == [[1, 1], [1, 1]] and residue.tolist() == [0, 0]
    else:
        assert counts.tolist() == [[1, 1], [0, 0]] and residue.tolist() == [0, 4]


def scatter(golhip, W, H, n, seed, seams, wrap):
    """n objects of common_objects() on a W x H board, their rings not overlapping, the first ones at
    the given places (the top-left corner of the ring); plus an R-pentomino.  wrap: objects may lie
    across the board's seams; else only a ring may hang out, by its one cell.  Returns the board."""
    rng = np.random.default_rng(seed)
    arrays = [a for v in golhip.common_objects().values() for a in v]
    board = np.zeros((H, W), dtype=np.uint8)
    used = np.zeros((H, W), dtype=bool)

    def place(a, x, y):
        h, w = a.shape
        if not wrap and not (-1 <= x and x + w - 1 <= W and -1 <= y and y + h - 1 <= H):
            return False
        rows, cols = np.arange(h) + y, np.arange(w) + x
        if not wrap:  # the part of a ring that hangs out takes no room
            rows, cols = rows[(rows >= 0) & (rows < H)], cols[(cols >= 0) & (cols < W)]
        ys, xs = np.ix_(rows % H, cols % W)
        if used[ys, xs].any():
            return False
        used[ys, xs] = True
        put(board, a, x, y)
        return True

    assert place(np.pad(RPENT, 1), 200, 300)
    placed = 0
    for x, y in seams:
        placed += place(arrays[placed % len(arrays)], x, y)
    assert placed == len(seams)
    while placed < n:
        a = arrays[int(rng.integers(len(arrays)))]
        placed += place(a, int(rng.integers(-1, W)), int(rng.integers(-1, H)))
    return board


@pytest.mark.parametrize("topology", ["torus", "plane"])
def test_5_the_largest_frame(golhip, topology):
    """One 512 x 512 board: 200 isolated objects, some across the row and column seams and across
    word seams, and an R-pentomino that nothing explains."""
    W = H = 512
    if topology == "torus":  # across the column seam, the row seam, the corner, and three word seams
        seams = [(510, 40), (509, 100), (60, 510), (130, 509), (510, 510), (30, 200), (62, 220), (254, 240)]
    else:  # at the borders with the ring outside, in two corners, and on three word seams
        seams = [(-1, 40), (100, -1), (-1, -1), (30, 200), (62, 220), (254, 240), (507, 507), (507, 60)]
    board = scatter(golhip, W, H, 200, 5, seams, topology == "torus")
    pats = [a for v in golhip.common_objects().values() for a in v]
    counts, residue = check(golhip, [board], pats, topology)
    assert counts.sum() >= 150 and residue[0] == 5


def test_6_overlaps_and_cells_not_looked_at(golhip):
    rng = np.random.default_rng(6)
    boards = (rng.random((3, 16, 64)) < 0.4).astype(np.uint8) * 255
    one = np.ones((1, 1), dtype=np.int8)
    for topology in ("torus", "plane"):
        counts, residue = check(golhip, boards, [one], topology)
        assert counts[:, 0].tolist() == (boards != 0).sum(axis=(1, 2)).tolist() and residue.tolist() == [0, 0, 0]
    sq = np.zeros((1, 16, 16), dtype=np.uint8)
    put(sq[0], np.ones((3, 3)), 5, 5)
    counts, residue = check(golhip, sq, [BLOCK], "torus")
    assert counts[0, 0] == 4 and residue[0] == 0
    # a block whose corner cell is not looked at: matches the block, and the block with that cell dead
    loose = np.array([[-1, 1], [1, 1]], dtype=np.int8)
    b = np.zeros((2, 16, 16), dtype=np.uint8)
    put(b[0], BLOCK, 2, 2)
    put(b[1], np.array([[0, 1], [1, 1]]), 9, 9)
    counts, residue = check(golhip, b, [loose, BLOCK], "plane")
    assert counts.tolist() == [[1, 1], [1, 0]] and residue.tolist() == [0, 0]
    counts, residue = check(golhip, b, [loose], "plane")
    assert counts.tolist() == [[1], [1]] and residue.tolist() == [1, 0]  # a cell not looked at is not covered


def test_7_residue(golhip):
    b = np.zeros((1, 32, 64), dtype=np.uint8)
    put(b[0], BLOCK, 4, 4)
    put(b[0], RPENT, 40, 20)
    counts, residue = check(golhip, b, [golhip.isolated(BLOCK)], "torus")
    assert counts[0, 0] == 1 and residue[0] == 5
    with golhip.Batch(64, 32, 1) as batch:
        batch.load(b)
        counts, residue = batch.census([])
        assert counts.shape == (1, 0) and residue.tolist() == batch.alive_counts().tolist() == [9]
        only, none = batch.census([golhip.isolated(BLOCK)], residue=False)
        assert none is None and only.tolist() == [[1]]
        none, only = batch.census([golhip.isolated(BLOCK)], counts=False)
        assert none is None and only.tolist() == [5]


@pytest.fixture(scope="module")
def ash_boards():
    return (np.random.default_rng(1).random((32, 64, 64)) < 0.5).astype(np.uint8) * 255


@pytest.mark.parametrize("topology", ["torus", "plane"])
def test_8_the_ash_of_32_soups(golhip, ash_boards, topology):
    """32 boards of 64 x 64 at density 1/2 run 2000 turns on the device: the census of the catalogue
    equals the reference's on the boards store() returns, and it is not vacuous."""
    objs = golhip.common_objects()
    names = [k for k, v in objs.items() for _ in v]
    pats = [a for v in objs.values() for a in v]
    with golhip.Batch(64, 64, 32, topology=topology) as b:
        b.load(ash_boards)
        b.step(2000)
        counts, residue = b.census(pats)
        boards = b.store()
    rc, rr = ref_all(boards, pats, topology)
    totals = {k: int(sum(counts[:, i].sum() for i, n in enumerate(names) if n == k)) for k in objs}
    print(topology, totals, "residue", residue.tolist())
    assert np.array_equal(counts, rc) and np.array_equal(residue, rr)
    assert totals["block"] > 0 and totals["blinker"] > 0 and totals["beehive"] > 0
    assert (residue == 0).any() and (residue != 0).any()


def test_9_256_patterns_in_one_call(golhip, ash_boards):
    pats = [a for v in golhip.common_objects().values() for a in v]
    rng = np.random.default_rng(9)
    order = rng.permutation(np.arange(256) % 33)
    many = [pats[i] for i in order]
    with golhip.Batch(64, 64, 8) as b:
        b.load(ash_boards[:8])
        b.step(600)
        singles = np.stack([b.census([p], residue=False)[0][:, 0] for p in pats], axis=1)
        base_counts, base_residue = b.census(pats)
        counts, residue = b.census(many)
        assert np.array_equal(base_counts, singles)
        assert np.array_equal(counts, singles[:, order])
        assert np.array_equal(residue, base_residue)
        again, residue2 = b.census([many[i] for i in rng.permutation(256)], counts=False)
        assert again is None and np.array_equal(residue2, base_residue)
        assert singles.sum() > 0
        with pytest.raises(golhip.GolHipError) as e:
            b.census(many + [pats[0]])
        assert e.value.code == golhip.ERR_ARG and "257" in str(e.value)


CHILD = """
import sys
sys.path.insert(0, {pkg!r})
import numpy as np
import golhip
boards = np.load({inp!r})
pats = [np.ones((1, 1), dtype=np.int8), golhip.isolated(np.ones((1, 1), dtype=np.int8))] + list(np.load({pat!r}))
with golhip.Batch(boards.shape[2], boards.shape[1], boards.shape[0], topology={topology!r}) as b:
    b.load(boards)
    counts, residue = b.census(pats[:{npat}])
    np.savez({out!r}, counts=counts, residue=residue)
"""


def test_10_more_boards_than_a_launch(golhip, tmp_path):
    """70 000 boards of 4 x 4: two launches.  The 1 x 1 pattern and a lone cell in its ring, exact for
    every board; and the same from a fresh process whose transfer stage is as small as it gets, one
    word per board (GOLHIP_STAGE_BYTES): four launches."""
    n = 70000
    boards = (np.random.default_rng(10).random((n, 4, 4)) < 0.15).astype(np.uint8) * 255
    one = np.ones((1, 1), dtype=np.int8)
    lone = np.pad(one, 1)
    # the reference, vectorised over the boards: a lone cell has 8 dead neighbours on the torus
    a = boards != 0
    nb = sum(np.roll(np.roll(a, dr, 1), dc, 2) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr, dc) != (0, 0))
    want = np.stack([a.sum(axis=(1, 2)), (a & (nb == 0)).sum(axis=(1, 2))], axis=1)
    for i in (0, 1, 65535, 65536, n - 1):  # and the brute force itself on a few
        rc, rr = ref_census(boards[i], [one, lone], "torus")
        assert rc.tolist() == want[i].tolist() and rr == 0
    with golhip.Batch(4, 4, n) as b:
        b.load(boards)
        counts, residue = b.census([one, lone])
        lone_counts, lone_residue = b.census([lone])
    assert np.array_equal(counts, want) and not residue.any()
    assert np.array_equal(lone_counts[:, 0], want[:, 1])
    assert np.array_equal(lone_residue, want[:, 0] - want[:, 1])
    np.save(tmp_path / "in.npy", boards)
    np.save(tmp_path / "pat.npy", np.zeros((0, 1, 1), dtype=np.int8))
    code = CHILD.format(pkg=str(PKG), inp=str(tmp_path / "in.npy"), pat=str(tmp_path / "pat.npy"),
                        out=str(tmp_path / "out.npz"), topology="torus", npat=2)
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, "-c", code], env=dict(os.environ, GOLHIP_STAGE_BYTES="1"), check=True,
                   timeout=120)
    small = np.load(tmp_path / "out.npz")
    assert np.array_equal(small["counts"], want) and not small["residue"].any()


def test_10b_a_stage_smaller_than_a_board_s_counts(golhip, ash_boards, tmp_path):
    """Three boards and a 64-byte stage: it does not hold one board's 33 counts and its residue, so the
    counts come back in groups of 16 patterns, a board per launch, and the residue in a pass of its
    own over the whole list."""
    pats = [a for v in golhip.common_objects().values() for a in v]
    with golhip.Batch(64, 64, 3, topology="plane") as b:
        b.load(ash_boards[:3])
        b.step(500)
        boards = b.store()
        want_counts, want_residue = b.census(pats)
    np.save(tmp_path / "in.npy", boards)
    np.save(tmp_path / "pat.npy", np.zeros((0, 1, 1), dtype=np.int8))
    code = CHILD.format(pkg=str(PKG), inp=str(tmp_path / "in.npy"), pat=str(tmp_path / "pat.npy"),
                        out=str(tmp_path / "out.npz"), topology="plane", npat=2)
    code = code.replace("pats[:2]", "[a for v in golhip.common_objects().values() for a in v]")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, "-c", code], env=dict(os.environ, GOLHIP_STAGE_BYTES="1"), check=True,
                   timeout=120)
    small = np.load(tmp_path / "out.npz")
    assert np.array_equal(small["counts"], want_counts) and np.array_equal(small["residue"], want_residue)
    rc, rr = ref_all(boards, pats, "plane")
    assert np.array_equal(want_counts, rc) and np.array_equal(want_residue, rr)


def test_11_nothing_else_moves(golhip, ash_boards):
    pats = [a for v in golhip.common_objects().values() for a in v]
    rules = [("B3/S23", "B36/S23")[i % 2] for i in range(6)]
    with golhip.Batch(64, 64, 6, rules=rules, topology="plane", soup_box=(20, 12)) as b, \
            golhip.Batch(64, 64, 6, rules=rules, topology="plane", soup_box=(20, 12)) as quiet:
        for batch in (b, quiet):
            batch.load(ash_boards[:6])
            batch.track_period()
            batch.step(100)
        before = (b.store(), b.turn, b.periods(), b.rules, b.topology, b.soup_box, b.kernel_form)
        counts, residue = b.census(pats)
        after = (b.store(), b.turn, b.periods(), b.rules, b.topology, b.soup_box, b.kernel_form)
        assert before[1] == after[1] == 100 and before[4:] == after[4:] == ("plane", (20, 12), 3)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[3], after[3])
        assert all(np.array_equal(x, y) for x, y in zip(before[2], after[2]))
        rc, rr = ref_all(after[0], pats, "plane")
        assert np.array_equal(counts, rc) and np.array_equal(residue, rr)
        b.step(157)
        quiet.step(157)
        assert np.array_equal(b.store(), quiet.store()) and b.turn == quiet.turn == 257
        assert all(np.array_equal(x, y) for x, y in zip(b.periods(), quiet.periods()))
        b.track_period(False)  # and with tracking off, at another turn
        counts, residue = b.census(pats)
        rc, rr = ref_all(b.store(), pats, "plane")
        assert np.array_equal(counts, rc) and np.array_equal(residue, rr)


def bad_patterns(golhip):
    """(what, patterns, the index the text must name or None, a word of the offence)."""
    P = golhip.Pattern
    good = golhip.pattern(golhip.isolated(BLOCK))

    def make(w, h, alive, care):
        p = P(w=w, h=h)
        for r, (a, c) in enumerate(zip(alive, care)):
            p.alive[r], p.care[r] = a, c
        return p

    wide = make(32, 2, [1, 0], [0xFFFFFFFF, 0xFFFFFFFF])
    tall = make(2, 32, [1] * 32, [3] * 32)
    return [
        ("w == 0", [good, make(0, 2, [1], [1])], 1, "1..32"),
        ("w == 33", [make(33, 2, [1], [1])], 0, "1..32"),
        ("h == 0", [good, good, make(2, 0, [], [])], 2, "1..32"),
        ("h == 40", [good, make(2, 40, [1], [1])], 1, "1..32"),
        ("w > width", [good, wide], 1, "larger than"),
        ("h > height", [tall], 0, "larger than"),
        ("a bit at column >= w", [good, make(2, 2, [1, 0], [3, 7])], 1, "column"),
        ("a bit in a row >= h", [good, good, good, make(2, 2, [1, 0, 0], [3, 3, 1])], 3, "row 2"),
        ("alive outside care", [make(2, 2, [3, 0], [1, 3])], 0, "subset"),
        ("no live cell", [good, make(2, 2, [0, 0], [3, 3])], 1, "no live cell"),
    ]


def test_12_errors(golhip):
    boards = np.zeros((2, 16, 16), dtype=np.uint8)
    put(boards[0], BLOCK, 3, 3)
    lib = golhip.load_library()
    with golhip.Batch(16, 16, 2) as b:
        b.load(boards)
        b.step(3)
        for what, pats, index, word in bad_patterns(golhip):
            with pytest.raises(golhip.GolHipError) as e:
                b.census(pats)
            assert e.value.code == golhip.ERR_ARG, what
            assert f"pattern {index}" in str(e.value) and word in str(e.value), (what, str(e.value))
        # the C call itself: the outputs stay as they were filled
        import ctypes
        table = (golhip.Pattern * 2)(golhip.pattern(golhip.isolated(BLOCK)), golhip.Pattern(w=2, h=2))
        counts = np.full((2, 2), 77, dtype=np.uint32)
        residue = np.full(2, 88, dtype=np.uint32)
        h = b._h
        calls = [
            ("a pattern without a live cell", (ctypes.addressof(table), 2, counts.ctypes.data, residue.ctypes.data), "pattern 1"),
            ("npat < 0", (ctypes.addressof(table), -1, counts.ctypes.data, residue.ctypes.data), "-1"),
            ("npat > 256", (ctypes.addressof(table), 257, counts.ctypes.data, residue.ctypes.data), "257"),
            ("patterns == NULL", (None, 1, counts.ctypes.data, residue.ctypes.data), "null"),
            ("both outputs NULL", (ctypes.addressof(table), 1, None, None), "both null"),
        ]
        for what, args, word in calls:
            assert lib.golhip_batch_census(h, *args) == golhip.ERR_ARG, what
            assert word in lib.golhip_batch_last_error(h).decode(), what
            assert (counts == 77).all() and (residue == 88).all(), what
        with pytest.raises(golhip.GolHipError) as e:  # an array is refused before the library sees it
            b.census([golhip.isolated(BLOCK), np.zeros((3, 3))])
        assert e.value.code == golhip.ERR_ARG and "pattern 1" in str(e.value) and "no live cell" in str(e.value)
        # the handle is untouched: the turn, the boards, and a good call still works
        assert b.turn == 3 and np.array_equal(b.store(), boards)
        counts, residue = b.census([golhip.isolated(BLOCK)])
        assert counts.tolist() == [[1], [0]] and residue.tolist() == [0, 0]
