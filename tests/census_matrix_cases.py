"""The case table of tests/test_gpu_census_matrix.py: gol_batch_census at every width class, every
height, both topologies and every kind of pattern include/golhip.h allows, with the expected values
by numpy.  Plain Python, no GPU: tests/test_census_matrix_cpu.py pins np_census to the brute force of
tests/test_gpu_batch_census.py, checks that the table is complete and that no case is vacuous;
tests/test_gpu_census_matrix.py compares the kernel with it.

np_census is the reference: (counts, residue) of a stack of boards, from the definitions of
include/golhip.h, vectorised over boards and anchors.  It knows nothing of words, frames, lanes or
replicas.

A case is (width, height, topology, family): case(...) gives its boards (n, h, w; 1 = alive), its
patterns (arrays of 1 / 0 / -1) and what the family records about them; expected(...) caches
np_census of it (read-only arrays).  The families:

  sweep     one object alone on an empty board, one board per offset: an R-pentomino matched in its
            ring, bare, by its live cells alone, and a glider's ring that never matches; a cell and a
            domino where the ring does not fit (NO_RPENTOMINO)
  largest   patterns of min(32, width) x min(32, height) cut from random boards at bit 0, at bit 31
            and across the seams, a third of their cells not looked at; a row, a column, and a
            pattern that looks at columns 0 and 31 only
  skipped   the largest patterns with whole rows not looked at
  dense     16 random 3 x 3 patterns that look at 3 to 6 cells, 2 x 2 and 1 x 3 all alive, on soups of
            density 0.5, 0.2, 0.9
  selfwrap  widths 2 to 16: patterns as wide as the board, a full row on a board with one full row
  mixed     patterns that match nowhere, in one row only and all over, interleaved

Where a shape cannot meet a condition of tests/test_census_matrix_cpu.py the reason stands in one of
the dictionaries ONE_BOARD, NO_RPENTOMINO, NO_RING, FEW_ANCHORS, ALL_EXPLAINED, MOSTLY_SIGNATURE below, and the check names the shape.
"""
import functools

import numpy as np

TOPOLOGIES = ("torus", "plane")
MARGIN = 31  # a pattern has at most 32 rows and columns: the dead cells around a plane

# every width the engine accepts (narrow rows with 32, 16, 8, 4 and 2 replicas in a word, one word, 2,
# 4, 8 and 16 words) and every height; 64-lane workgroups (1 x 4 .. 512 x 4) and 1024-lane ones that
# loop (64 x 512 on the plane, 512 x 128); on a plane no item count is a multiple of the block size
SHAPES = [(1, 4), (2, 8), (4, 256), (8, 16), (16, 64), (32, 4), (32, 32), (64, 512), (128, 8), (256, 32), (512, 4),
          (512, 128), (512, 512)]
SHAPE_IDS = [f"{w}x{h}" for w, h in SHAPES]
FAMILIES = ("sweep", "largest", "skipped", "dense", "selfwrap", "mixed")

# 512 x 512: the reference needs a third of a second per 32 x 32 pattern there, so one board, the
# largest patterns only
ONE_BOARD = {(512, 512): "one board: a largest pattern has no other board to stay away from"}
# the R-pentomino in its ring is 5 x 5: these take a cell and a domino.  On the plane such a sweep has no
# board with residue > 0: a cell or a domino cut at the border is a cell or nothing, and the list that
# explains a lone cell on the torus explains it on the plane.  The condition there is that some board
# holds less than the object and the object's ring does not match it
NO_RPENTOMINO = {(1, 4): "1 wide", (2, 8): "2 wide", (4, 256): "4 wide", (32, 4): "4 rows", (512, 4): "4 rows"}
# a ring is 3 wide at the least.  Without one the sweep's condition is on the bare object
NO_RING = {(1, 4): "1 wide: no ring fits, the bare object counts once",
           (2, 8): "2 wide: no ring fits, the bare object counts once"}
# a count above 32 needs more than 32 anchors with a live cell under them
FEW_ANCHORS = {(1, 4): "4 cells", (2, 8): "16 cells"}
# the dense patterns are 3 x 1 there: 16 random ones are nearly all 7 there are, and explain every cell
ALL_EXPLAINED = {(1, 4): "3 x 1 patterns: every cell is explained, the residue is 0"}
# the mixed list's residue: the signature's three rows are most of so small a board, and the R patterns
# explain them
MOSTLY_SIGNATURE = {(1, 4): "4 cells", (2, 8): "16 cells", (8, 16): "128 cells", (32, 4): "128 cells"}

RPENT = np.array([[0, 1, 1], [1, 1, 0], [0, 1, 0]], dtype=np.int8)
GLIDER = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=np.int8)
CELL = np.ones((1, 1), dtype=np.int8)
DOMINO = np.ones((2, 1), dtype=np.int8)  # upright: it fits a board 1 wide


def families_of(shape):
    if shape in ONE_BOARD:
        return ("largest",)
    return tuple(f for f in FAMILIES if f != "selfwrap" or 2 <= shape[0] <= 16)


CASES = [(w, h, t, f) for (w, h) in SHAPES for t in TOPOLOGIES for f in families_of((w, h))]
CASE_IDS = [f"{w}x{h}-{t}-{f}" for w, h, t, f in CASES]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def ring(cells):
    """`cells` inside a ring of dead cells (golhip.isolated, written out: this module is plain numpy)."""
    return np.pad(np.asarray(cells, dtype=np.int8), 1)


# ------------------------------------------------------------------------------ the reference
def np_census(boards, patterns, topology):
    """(counts (n, npat), residue (n,)) of boards (n, h, w; nonzero = alive) by the definitions of
    include/golhip.h.  Per pattern the match array, one flag per anchor, is the AND over the cells the
    pattern looks at of `the board shifted by that cell == the cell`; the cover is the OR over the
    pattern's live cells of the match array shifted by that cell; the residue counts the live cells
    outside every cover.  A torus shifts with np.roll.  A plane is padded with 31 dead cells on
    every side, so that the anchors -(w - 1) .. width - 1 and -(h - 1) .. height - 1 are ordinary
    positions of the padded array and nothing a pattern reaches from them wraps; the other positions
    of the padded array are no anchors."""
    a = np.asarray(boards) != 0
    assert a.ndim == 3 and topology in TOPOLOGIES
    n, H, W = a.shape
    plane = topology == "plane"
    if plane:
        a = np.pad(a, ((0, 0), (MARGIN, MARGIN), (MARGIN, MARGIN)))
    counts = np.zeros((n, len(patterns)), dtype=np.int64)
    cover = np.zeros(a.shape, dtype=bool)
    for k, p in enumerate(patterns):
        p = np.asarray(p)
        h, w = p.shape
        assert 1 <= h <= min(32, H) and 1 <= w <= min(32, W) and (p == 1).any()
        match = np.ones(a.shape, dtype=bool)
        if plane:
            match[:] = False
            match[:, MARGIN - (h - 1):MARGIN + H, MARGIN - (w - 1):MARGIN + W] = True
        for r in range(h):
            if (p[r] < 0).all():
                continue
            rows = np.roll(a, -r, axis=1)  # rows[y] = a[y + r]
            for c in np.nonzero(p[r] >= 0)[0]:
                cell = np.roll(rows, -int(c), axis=2)  # cell[y, x] = a[y + r, x + c]
                match &= cell if p[r, c] == 1 else ~cell
        counts[:, k] = match.sum(axis=(1, 2))
        if match.any():
            for r, c in zip(*np.nonzero(p == 1)):
                cover |= np.roll(match, (int(r), int(c)), axis=(1, 2))  # anchor (x, y) covers (x + c, y + r)
    residue = (a & ~cover).sum(axis=(1, 2))  # outside a plane's rectangle nothing is alive
    return counts, residue.astype(np.int64)


# ------------------------------------------------------------------------------ the helpers
def rng_of(shape, family):
    return np.random.default_rng([shape[0], shape[1], FAMILIES.index(family)])


def soup(rng, n, shape, density):
    w, h = shape
    return (rng.random((n, h, w)) < density).astype(np.uint8)


def put(board, cells, x, y, topology):
    """The live cells of `cells`, its top-left corner at (x, y): wrapped on a torus, cut at the border
    of a plane (x and y may be negative there)."""
    H, W = board.shape
    for r, c in zip(*np.nonzero(np.asarray(cells) == 1)):
        yy, xx = y + int(r), x + int(c)
        if topology == "torus":
            board[yy % H, xx % W] = 1
        elif 0 <= yy < H and 0 <= xx < W:
            board[yy, xx] = 1


def cut(board, x, y, w, h):
    """The w x h cells of a board from (x, y) on, wrapped, as a pattern that looks at all of them."""
    H, W = board.shape
    return board[np.ix_((y + np.arange(h)) % H, (x + np.arange(w)) % W)].astype(np.int8)


def loosen(rng, p, share):
    """`share` of the cells of a pattern not looked at, a live cell kept."""
    p = p.copy()
    p[rng.random(p.shape) < share] = -1
    if not (p == 1).any():
        return None
    return p


# ------------------------------------------------------------------------------ the sweep
def sweep_offsets(shape, topology):
    """[(x, y)]: where the object's top-left corner goes, one board each.  x: min(width, 70) values
    from width - 35 on, y: height - 3 .. height + 2, both taken mod the side (so on a plane the object
    is cut at the right and bottom border, and lies at 0 with its ring outside); every pair where
    that is at most 96 boards, else the x in turn with the y cycling.  On a plane five more with the
    object across the left and top border, which mod never gives."""
    w, h = shape
    xs = [(w - 35 + i) % w for i in range(min(w, 70))]
    ys = [(h - 3 + i) % h for i in range(6)]
    extra = [(-1, 1), (-2, h - 2), (5 % w, -1), (w - 2, -2), (-1, -1)] if topology == "plane" else []
    if len(xs) * 6 + len(extra) <= 96 // (2 if w < 5 else 1):
        return [(x, y) for x in xs for y in ys] + extra
    return [(x, ys[i % 6]) for i, x in enumerate(xs)] + extra


def sweep_case(shape, topology):
    """meta: ringed[i] = the pattern that is board i's object in its ring (None where no ring fits:
    NO_RING), bare[i] = the object bare."""
    w, h = shape
    offsets = sweep_offsets(shape, topology)
    if shape not in NO_RPENTOMINO:
        boards = np.zeros((len(offsets), h, w), dtype=np.uint8)
        for b, (x, y) in zip(boards, offsets):
            put(b, RPENT, x, y, topology)
        patterns = [ring(RPENT), RPENT, np.where(RPENT == 1, 1, -1).astype(np.int8), ring(GLIDER)]
        ringed, bare = [0] * len(offsets), [1] * len(offsets)
    else:
        # a cell and a domino.  5 columns or more (then 4 rows): both on every board, half a board
        # apart; narrower: a board each
        patterns = [CELL, DOMINO] + ([ring(CELL), ring(DOMINO)] if w >= 3 else [])
        if w >= 5:
            boards = np.zeros((len(offsets), h, w), dtype=np.uint8)
            for b, (x, y) in zip(boards, offsets):
                put(b, DOMINO, x, y, topology)
                put(b, CELL, (x + w // 2) % w, y % h, topology)
            ringed, bare = [3] * len(offsets), [1] * len(offsets)
        else:
            boards = np.zeros((2 * len(offsets), h, w), dtype=np.uint8)
            for i, (x, y) in enumerate(offsets):
                put(boards[2 * i], CELL, x, y, topology)
                put(boards[2 * i + 1], DOMINO, x, y, topology)
            ringed, bare = [2, 3] * len(offsets), [0, 1] * len(offsets)
        if w < 3:
            ringed = None
    return boards, patterns, {"ringed": ringed, "bare": bare, "offsets": offsets}


# ------------------------------------------------------------------------------ the largest patterns
def largest_anchors(shape, topology):
    """Bit 0 of a word, bit 31 of a word (the last column of a narrower board), and across the right
    and bottom seams; on a plane each moved back to where the pattern still lies inside."""
    w, h = shape
    pw, ph = min(32, w), min(32, h)
    anchors = [(32 if w >= 64 else 0, 1), (min(31, w - 1), 2), (w - max(pw // 2, 1), h - ph // 2)]
    if topology == "plane":
        anchors = [(min(x, w - pw), min(y, h - ph)) for x, y in anchors]
    return anchors


@functools.lru_cache(maxsize=None)
def largest_boards(shape):
    """Three soups of density 0.5 the patterns are cut from and one they are not; below 256 cells a
    pattern is small enough to match any soup, so an empty board too.  The cell under each anchor is
    alive: every cut has a live cell."""
    boards = soup(rng_of(shape, "largest"), 1 if shape in ONE_BOARD else 4, shape, 0.5)
    for topology in TOPOLOGIES:
        for j, (x, y) in enumerate(largest_anchors(shape, topology)):
            boards[j % boards.shape[0], y % shape[1], x % shape[0]] = 1
    if shape in ONE_BOARD:
        return frozen(boards)
    if shape[0] * shape[1] < 256:
        boards = np.concatenate([boards, np.zeros_like(boards[:1])])
    return frozen(boards)


@functools.lru_cache(maxsize=None)
def largest_patterns(shape, topology):
    """([pattern], [its board]) of the three largest patterns."""
    w, h = shape
    pw, ph = min(32, w), min(32, h)
    boards = largest_boards(shape)
    rng = np.random.default_rng([w, h, 99, TOPOLOGIES.index(topology)])
    pats, owners = [], []
    for j, (x, y) in enumerate(largest_anchors(shape, topology)):
        owner = j % boards.shape[0]
        full = cut(boards[owner], x, y, pw, ph)
        p = None
        for _ in range(64):  # a third of the cells not looked at; on a tiny board until a live cell is left
            p = loosen(rng, full, 1 / 3)
            if p is not None and (pw < 32 or ((p[:, 0] >= 0).any() and (p[:, 31] >= 0).any())):
                break
        else:
            p = full
        pats.append(frozen(p))
        owners.append(owner)
    return pats, owners


def largest_case(shape, topology):
    """meta: owner[k] = the board pattern k was cut from."""
    w, h = shape
    pw, ph = min(32, w), min(32, h)
    boards = largest_boards(shape)
    pats, owners = largest_patterns(shape, topology)
    pats, owners = list(pats), list(owners)
    anchors = largest_anchors(shape, topology)
    # a row of min(32, width) cells and a column of min(32, height), every cell looked at
    (x0, y0), (x1, y1) = anchors[0], anchors[1]
    for p in (cut(boards[0], x1, y0, pw, 1), cut(boards[0], x0, y1, 1, ph)):
        if (p == 1).any():
            pats.append(p)
            owners.append(0)
    if w >= 32:  # columns 0 and 31 only, three rows: many matches, every one a shift by 31
        edge = cut(boards[owners[1]], x1, y1, 32, min(3, h))
        edge[:, 1:31] = -1
        if (edge == 1).any():
            pats.append(edge)
            owners.append(owners[1])
    return boards, pats, {"owner": owners}


def skipped_case(shape, topology):
    """Each largest pattern with row 0, two adjacent middle rows, the last row, and all of them not
    looked at; the pattern keeps its height.  A variant without a live cell is no pattern and is
    left out.  meta: owner[k], rows[k] = the rows cleared."""
    ph = min(32, shape[1])
    pats, owners, rows = [], [], []
    base, base_owner = largest_patterns(shape, topology)
    for p, owner in zip(base, base_owner):
        for cleared in ((0,), (ph // 2 - 1, ph // 2), (ph - 1,), (0, ph // 2 - 1, ph // 2, ph - 1)):
            q = p.copy()
            q[list(cleared)] = -1
            if (q == 1).any():
                pats.append(q)
                owners.append(owner)
                rows.append(cleared)
    return largest_boards(shape), pats, {"owner": owners, "rows": rows}


# ------------------------------------------------------------------------------ dense overlaps
def dense_case(shape, topology):
    """24 soups, 8 each of density 0.5, 0.2 and 0.9 (4 each from 2^15 cells on); 16 random patterns of
    3 rows and min(3, width) columns that look at 3 to 6 cells (all 3 of a 3 x 1), one of them alive at
    the least, a 2 x 2 and a row of 3 all alive (a column on a board too narrow for a row)."""
    w, h = shape
    rng = rng_of(shape, "dense")
    each = 4 if w * h >= 1 << 15 else 8
    boards = np.concatenate([soup(rng, each, shape, d) for d in (0.5, 0.2, 0.9)])
    pw = min(3, w)
    pats = []
    while len(pats) < 16:
        # most look at 6 cells, one each at 3, 4 and 5: a pattern that looks at few cells matches all
        # over, and a list of such explains every cell, which leaves the residue nothing to show
        p = rng.integers(0, 2, size=(3, pw)).astype(np.int8)
        cared = {3: 3, 7: 4, 11: 5}.get(len(pats), 6)
        drop = rng.permutation(3 * pw)[:max(3 * pw - cared, 0)]
        p.reshape(-1)[drop] = -1
        if (p == 1).any():
            pats.append(p)
    if w >= 2:
        pats.append(np.ones((2, 2), dtype=np.int8))
    pats.append(np.ones((1, 3) if w >= 3 else (3, 1), dtype=np.int8))
    return boards, pats, {}


def dense_patterns(shape):
    return dense_case(shape, "torus")[1]


# ------------------------------------------------------------------------------ self-wrap
def selfwrap_case(shape, topology):
    """Widths 2 to 16.  Six soups, a board with one full row, a board all alive.  Patterns exactly
    `width` wide, cut from the soups at three anchors (wrapped, so on a plane only the first lies as
    it was cut), min(32, height) and 2 rows tall, a quarter of the cells not looked at; a full row of
    `width` cells, and two full rows.  meta: full_row = the board with one full row, row = the
    index of the full-row pattern."""
    w, h = shape
    rng = rng_of(shape, "selfwrap")
    boards = np.concatenate([soup(rng, 6, shape, 0.5), np.zeros((1, h, w), np.uint8), np.ones((1, h, w), np.uint8)])
    boards[6, h // 2 + 1] = 1
    pats = []
    for j, (x, y) in enumerate([(0, 0), (w // 2 + 1, 1), (w - 1, h - 2)]):
        for ph in (min(32, h), 2):
            full = cut(boards[j], x, y, w, ph)
            p = loosen(rng, full, 1 / 4)
            p = full if p is None else p
            if (p == 1).any():
                pats.append(p)
    row = len(pats)
    pats += [np.ones((1, w), dtype=np.int8), np.ones((2, w), dtype=np.int8)]
    return boards, pats, {"full_row": 6, "row": row}


# ------------------------------------------------------------------------------ mixed early-out
def mixed_case(shape, topology):
    """Eight soups of density 0.3 that share three rows, the signature, from row height / 2 - 1 on.
    N patterns match nowhere: a 5 x 5 all alive, the first R pattern with one cell of its last row
    turned over (it fails in its last row where R matches, in its first elsewhere), a 3 x 3 all
    alive in its ring.  R patterns are cut from the signature, min(32, width) wide: from 32 columns
    on they match once per board, in the signature's row.  E patterns match all over: a live cell left of
    a dead one, a live cell two rows under a dead one (the row between not looked at), two live cells
    on a diagonal; none explains every cell, so the residue is not 0.  The list interleaves
    them.  meta: kinds = "N" / "R" / "E" per pattern, row = the signature's first row."""
    w, h = shape
    rng = rng_of(shape, "mixed")
    boards = soup(rng, 8, shape, 0.3)
    y0, sh = h // 2 - 1, min(3, h)
    sig = soup(rng, 1, (w, sh), 0.5)[0]
    sig[0, 0] = 1  # a live cell in every cut below
    boards[:, y0:y0 + sh] = sig
    pw = min(32, w)
    xs = [0, 31 if w >= 64 else w // 2, w - pw // 2 if topology == "torus" else w - pw]
    R = [cut(boards[0], x, y0, pw, sh) for x in xs]
    for p in R:
        if not (p == 1).any():
            p[0, 0] = 1  # then it is no cut any more and may match nowhere: the conditions do not need it
    late = R[0].copy()
    late[sh - 1, pw - 1] ^= 1
    N = [np.ones((min(5, h), min(5, w)), dtype=np.int8), late]
    if w >= 5 and h >= 5:
        N.append(ring(np.ones((3, 3), dtype=np.int8)))
    E = [np.array([[1, 0]] if w >= 2 else [[1], [0]], dtype=np.int8), np.array([[0], [-1], [1]], dtype=np.int8)]
    if w >= 2:
        E.append(np.array([[1, -1], [-1, 1]], dtype=np.int8))
    pats, kinds = [], []
    for i in range(3):
        for kind, group in (("N", N), ("R", R), ("E", E)):
            if i < len(group):
                pats.append(group[i])
                kinds.append(kind)
    return boards, pats, {"kinds": kinds, "row": y0}


# ------------------------------------------------------------------------------ the table
BUILDERS = {"sweep": sweep_case, "largest": largest_case, "skipped": skipped_case, "dense": dense_case,
            "selfwrap": selfwrap_case, "mixed": mixed_case}


@functools.lru_cache(maxsize=None)
def case(width, height, topology, family):
    """(boards (n, h, w) uint8 of 0 / 1, [pattern], meta), read-only."""
    assert (width, height, topology, family) in CASES
    boards, patterns, meta = BUILDERS[family]((width, height), topology)
    boards = boards if not boards.flags.writeable else frozen(np.ascontiguousarray(boards, dtype=np.uint8))
    patterns = [p if not p.flags.writeable else frozen(np.ascontiguousarray(p, dtype=np.int8)) for p in patterns]
    assert boards.shape[1:] == (height, width) and 1 <= boards.shape[0] <= 96 and 1 <= len(patterns) <= 24
    return boards, patterns, meta


@functools.lru_cache(maxsize=None)
def expected(width, height, topology, family):
    """(counts (n, npat), residue (n,)) of the case by np_census, read-only."""
    boards, patterns, _ = case(width, height, topology, family)
    return frozen(*np_census(boards, patterns, topology))
