"""The case table of tests/test_gpu_batch_objects.py and the reference it compares with: np_objects,
written from the definitions of include/golhip.h (cluster, order, extent, hash, record) alone.  Plain
Python and numpy, no GPU: tests/test_batch_objects_cpu.py checks that the table is complete, that no case
is vacuous and that np_objects itself meets each family's conditions; tests/test_gpu_batch_objects.py
compares gol_batch_objects with it, exactly.

np_objects is a flood fill from the row-major first cell over a set of live cells, occupancies by
any(), the hash in uint64 arithmetic.  It knows nothing of words, frames, lanes or replicas.

A case is (width, height, topology, family, reach); case(...) gives its boards (n, h, w; 1 = alive)
and what the family records about them, expected(...) caches np_objects of it.  The families:

  sweep   one R-pentomino alone on a board -- a domino where a side is below 8 -- at every x offset in
          rows 0, 1 and height - 1 and at every y offset in columns 0 and 31: wrapped on a torus,
          cut at the border of a plane
  gap     two cells at distance reach and reach + 1 along x, along y and on the diagonal, inside a
          word, across a word seam and across the torus seam (the second cell is placed mod the
          side on either topology: on a plane the two then lie at opposite borders)
  winds   a full row, a full column, the full board, a dotted row with gaps of reach - 1 and one with
          gaps of reach
  soup    random boards of density 0.5, 0.2 and 0.04
  snake   64 x 64, a shape beside the 13: one serpentine cluster along the rows and one along the
          columns, and each cut in two by one dead cell
  cap     16 x 64 and 64 x 512 only: a grid of isolated cells, more clusters than max_objects

512 x 512 has one board per case (ONE_BOARD): the sweep's object across the corner at (510, 510), one
board that holds the winds family's row and column, one sparse soup; the gap family needs its boards
and is left out.
"""
import functools

import numpy as np

import census_matrix_cases as census_cases

TOPOLOGIES = census_cases.TOPOLOGIES
SHAPES = census_cases.SHAPES
SHAPE_IDS = census_cases.SHAPE_IDS
REACHES = (1, 2)
WINDS_X, WINDS_Y, AT_BORDER = 1, 2, 4
OBJECT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("population", "<i4"),
                         ("flags", "<u4"), ("hash", "<u8")])

ONE_BOARD = {(512, 512): "one board per case: the reference floods it in Python"}
SNAKE_SHAPE = (64, 64)
CAP_SHAPES = ((16, 64), (64, 512))
CAP_LIMITS = (1, 7)
FAMILIES = ("sweep", "gap", "winds", "soup", "snake", "cap")

RPENT = census_cases.RPENT
DOMINO = census_cases.DOMINO


def families_of(shape):
    out = ["sweep", "winds", "soup"]
    if shape not in ONE_BOARD:
        out.insert(1, "gap")
    if shape in CAP_SHAPES:
        out.append("cap")
    return tuple(out)


CASES = [(w, h, t, f, r) for (w, h) in SHAPES for t in TOPOLOGIES for f in families_of((w, h)) for r in REACHES]
# the snake has a shape of its own, 64 x 64, beside the 13
CASES += [(SNAKE_SHAPE[0], SNAKE_SHAPE[1], t, "snake", r) for t in TOPOLOGIES for r in REACHES]
CASE_IDS = [f"{w}x{h}-{t}-{f}-reach{r}" for w, h, t, f, r in CASES]


# ------------------------------------------------------------------------------ the reference
def mix(v):
    """The splitmix64 finaliser on an array of uint64 (the arithmetic wraps mod 2^64)."""
    with np.errstate(over="ignore"):
        z = v.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def shape_hash(dx, dy, w, h):
    """The smallest H_k of the cells at the places (dx, dy) of a w x h box."""
    dx, dy = np.asarray(dx, dtype=np.uint64), np.asarray(dy, dtype=np.uint64)
    ex, ey = np.uint64(w - 1) - dx, np.uint64(h - 1) - dy
    best = None
    for k, (u, v) in enumerate([(dx, dy), (ex, dy), (dx, ey), (ex, ey), (dy, dx), (ey, dx), (dy, ex), (ey, ex)]):
        ow, oh = (w, h) if k < 4 else (h, w)
        with np.errstate(over="ignore"):
            total = mix((v << np.uint64(16)) | u).sum(dtype=np.uint64)
        hk = int(total) ^ int(mix(np.array([1 << 32 | oh << 16 | ow], dtype=np.uint64))[0])
        best = hk if best is None or hk < best else best
    return best


def axis_extent(occupied, cyclic, reach):
    """(x0, w, winds) of a boolean occupancy along one axis."""
    n = len(occupied)
    idx = np.nonzero(occupied)[0]
    if not cyclic:
        return int(idx[0]), int(idx[-1] - idx[0] + 1), False
    # the cyclic runs of empty places: between consecutive occupied places, the last one wraps to the first
    runs = []
    for a, b in zip(idx, np.roll(idx, -1)):
        length = (int(b) - int(a) - 1) % n if len(idx) > 1 else n - 1
        if length >= reach:
            runs.append((int(a), length))
    assert len(runs) <= 1, "a connected cluster has at most one such run"
    if not runs:
        return 0, n, True
    a, length = runs[0]
    return (a + length + 1) % n, n - length, False


def board_objects(board, topology, reach):
    """The records of one board (h, w; nonzero = alive), in the order of the definition."""
    H, W = board.shape
    torus = topology == "torus"
    ys, xs = np.nonzero(board)
    cells = list(zip(xs.tolist(), ys.tolist()))  # row-major: np.nonzero goes row by row
    left = set(cells)
    offsets = [(a, b) for b in range(-reach, reach + 1) for a in range(-reach, reach + 1) if (a, b) != (0, 0)]
    out = []
    for first in cells:
        if first not in left:
            continue
        left.discard(first)
        cluster, stack = [first], [first]
        while stack:
            x, y = stack.pop()
            for a, b in offsets:
                xx, yy = x + a, y + b
                if torus:
                    xx, yy = xx % W, yy % H
                elif not (0 <= xx < W and 0 <= yy < H):
                    continue
                if (xx, yy) in left:
                    left.discard((xx, yy))
                    cluster.append((xx, yy))
                    stack.append((xx, yy))
        cx = np.array([c[0] for c in cluster])
        cy = np.array([c[1] for c in cluster])
        occ_x, occ_y = np.zeros(W, dtype=bool), np.zeros(H, dtype=bool)
        occ_x[cx], occ_y[cy] = True, True
        x0, w, wx = axis_extent(occ_x, torus, reach)
        y0, h, wy = axis_extent(occ_y, torus, reach)
        flags = (WINDS_X if wx else 0) | (WINDS_Y if wy else 0)
        if not torus and (cx.min() == 0 or cx.max() == W - 1 or cy.min() == 0 or cy.max() == H - 1):
            flags |= AT_BORDER
        out.append((x0, y0, w, h, len(cluster), flags, shape_hash((cx - x0) % W, (cy - y0) % H, w, h)))
    return out


def np_objects(boards, topology, reach):
    """[the records of board i] of boards (n, h, w; nonzero = alive), each a structured array of
    OBJECT_DTYPE in the order of the definition."""
    assert topology in TOPOLOGIES and reach in REACHES
    boards = np.asarray(boards)
    assert boards.ndim == 3
    return [np.array(board_objects(b, topology, reach), dtype=OBJECT_DTYPE) for b in boards]


# ------------------------------------------------------------------------------ the helpers
put = census_cases.put
frozen = census_cases.frozen


def rng_of(shape, family, reach):
    return np.random.default_rng([shape[0], shape[1], FAMILIES.index(family), reach, 15])


def sweep_object(shape):
    return RPENT if min(shape) >= 8 else DOMINO


# ------------------------------------------------------------------------------ the families
def sweep_case(shape, topology, reach):
    """meta: offsets[i] = where board i's object has its top-left corner, whole[i] = it lies inside
    the rectangle (always on a torus), obj = the object."""
    w, h = shape
    obj = sweep_object(shape)
    oh, ow = obj.shape
    if shape in ONE_BOARD:
        offsets = [(w - 2, h - 2)]
    else:
        offsets = [(x, y) for y in sorted({0, 1, h - 1}) for x in range(w)]
        offsets += [(x, y) for x in sorted({0, min(31, w - 1)}) for y in range(h)]
    boards = np.zeros((len(offsets), h, w), dtype=np.uint8)
    for b, (x, y) in zip(boards, offsets):
        put(b, obj, x, y, topology)
    whole = [topology == "torus" or (x + ow <= w and y + oh <= h) for x, y in offsets]
    return boards, {"offsets": offsets, "whole": whole, "obj": obj}


def gap_case(shape, topology, reach):
    """meta: pairs[i] = ((x, y), (x2, y2), d, (sx, sy)) of board i: the two cells, their distance along
    the direction (sx, sy) before the second was taken mod the sides."""
    w, h = shape
    xs = sorted({min(1, w - 1), 31 if w >= 64 else w // 2, w - 1})
    ys = sorted({min(1, h - 1), h - 1})
    pairs = []
    for d in (reach, reach + 1):
        for sx, sy in ((1, 0), (0, 1), (1, 1)):
            for x in xs:
                for y in ys:
                    pairs.append(((x, y), ((x + sx * d) % w, (y + sy * d) % h), d, (sx, sy)))
    boards = np.zeros((len(pairs), h, w), dtype=np.uint8)
    for b, (p, q, _, _) in zip(boards, pairs):
        b[p[1], p[0]] = 1
        b[q[1], q[0]] = 1
    return boards, {"pairs": pairs}


def winds_case(shape, topology, reach):
    """meta: kinds[i] of board i: "row", "column", "board", "dotted-linked" (gaps of reach - 1),
    "dotted-apart" (gaps of reach); "cross" for the one board of 512 x 512 (a row and a column)."""
    w, h = shape
    row, col = min(1, h - 1), min(31, w - 1)
    if shape in ONE_BOARD:
        board = np.zeros((1, h, w), dtype=np.uint8)
        board[0, row, :] = 1
        board[0, :, col] = 1
        board[0, h // 2, ::reach + 1] = 1
        return board, {"kinds": ["cross"]}
    boards = np.zeros((5, h, w), dtype=np.uint8)
    boards[0, row, :] = 1
    boards[1, :, col] = 1
    boards[2] = 1
    boards[3, row, ::reach] = 1
    boards[4, row, ::reach + 1] = 1
    return boards, {"kinds": ["row", "column", "board", "dotted-linked", "dotted-apart"]}


def soup_case(shape, topology, reach):
    w, h = shape
    rng = rng_of(shape, "soup", reach)
    if shape in ONE_BOARD:  # sparse, and two large pieces: a filled square and a long diagonal
        board = (rng.random((1, h, w)) < 0.01).astype(np.uint8)
        board[0, 100:140, 200:260] = 1
        board[0, np.arange(300, 500), np.arange(10, 210)] = 1
        return board, {}
    each = 2 if w * h >= 1 << 14 else 4
    boards = np.concatenate([(rng.random((each, h, w)) < d).astype(np.uint8) for d in (0.5, 0.2, 0.04)])
    return boards, {}


def snake_board(reach, cut):
    """A serpentine along the rows of a 64 x 64 board inside a margin of 3 dead cells: full rows
    every reach + 1 rows, joined at alternating ends by the cells between them."""
    b = np.zeros((64, 64), dtype=np.uint8)
    rows = list(range(3, 61, reach + 1))
    for i, y in enumerate(rows):
        b[y, 3:61] = 1
        if i + 1 < len(rows):
            b[y:rows[i + 1], 60 if i % 2 == 0 else 3] = 1
    if cut:
        b[rows[len(rows) // 2], 31] = 0
    return b


def snake_case(shape, topology, reach):
    assert shape == SNAKE_SHAPE
    boards = np.stack([snake_board(reach, False), snake_board(reach, False).T.copy(), snake_board(reach, True),
                       snake_board(reach, True).T.copy()])
    return boards, {"kinds": ["rows", "columns", "rows-cut", "columns-cut"]}


def cap_case(shape, topology, reach):
    """One board: a cell at every fourth column of every fourth row (every column below 4 wide)."""
    w, h = shape
    board = np.zeros((1, h, w), dtype=np.uint8)
    board[0, ::4, ::4] = 1
    return board, {"clusters": (h // 4) * max(w // 4, 1)}


BUILDERS = {"sweep": sweep_case, "gap": gap_case, "winds": winds_case, "soup": soup_case, "snake": snake_case,
            "cap": cap_case}


@functools.lru_cache(maxsize=None)
def case(width, height, topology, family, reach):
    """(boards (n, h, w) uint8 of 0 / 1, meta), read-only."""
    assert (width, height, topology, family, reach) in CASES
    boards, meta = BUILDERS[family]((width, height), topology, reach)
    boards = frozen(np.ascontiguousarray(boards, dtype=np.uint8))
    assert boards.shape[1:] == (height, width) and boards.shape[0] >= 1
    return boards, meta


@functools.lru_cache(maxsize=None)
def expected(width, height, topology, family, reach):
    """np_objects of the case, read-only."""
    boards, _ = case(width, height, topology, family, reach)
    return [frozen(r) for r in np_objects(boards, topology, reach)]


def table(records, max_objects):
    """(nobjects (n,), objects (n, max_objects)) as Batch.objects returns them, rows beyond a board's
    records zeros, from np_objects' list."""
    n = np.array([len(r) for r in records], dtype=np.int32)
    o = np.zeros((len(records), max_objects), dtype=OBJECT_DTYPE)
    for i, r in enumerate(records):
        m = min(len(r), max_objects)
        o[i, :m] = r[:m]
    return n, o
