"""Windowed board access on the GPU: golhip_store_rect / golhip_load_rect (a rectangle of the running
board as bytes, out and in) and golhip_view_counts / golhip_view (the density viewport: one pixel per
scale x scale block of cells), through single strips, multi-strip handles, the ring of one, two
ranks over the host transport, another rule and the host CLI.

Everything is bit-exact against numpy: np.roll + slice for rectangles, a block sum of the rolled
board for the viewport (pinned without a GPU in tests/test_rect_cpu.py), the oracle (B3/S23) or the
numpy rule stepper for what a stamped board becomes.  The board shapes are the ones where the
packed layout changes: 16x16 (torus of 128 columns = 8 horizontal replicas), 48x37 (3 words, 8
replicas, odd height), 64x64 (2 replicas), 2048x40 (no replica), 4000x24 (4 replicas, a ragged last
16-cell group).

Reference roles: sdl/loop.go (the window showing the world), gol/distributor.go:93-103 (the `s`
key's whole-world PGM), gol/io.go:42-128.
"""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import PKG, REF, ROOT

pytestmark = pytest.mark.gpu

BOARDS = [(16, 16), (48, 37), (64, 64), (2048, 40), (4000, 24)]  # (width, height)
MODES = ["copy", "or", "xor"]
GLIDER = np.array([[0, 255, 0], [0, 0, 255], [255, 255, 255]], np.uint8)


# ---------------------------------------------------------------- the numpy reference
@functools.lru_cache(maxsize=None)
def random_board(w, h, seed=0, density=0.5):
    b = np.where(np.random.default_rng(1000 * w + h + seed).random((h, w)) < density, 255, 0).astype(np.uint8)
    b.setflags(write=False)
    return b


def torus_index(board, x, y, w, h):
    H, W = board.shape
    return np.ix_((np.arange(h) + y) % H, (np.arange(w) + x) % W)


def np_rect(board, x, y, w, h):
    return board[torus_index(board, x, y, w, h)]


def np_edit(board, x, y, cells, mode):
    out = board.copy()
    ix = torus_index(board, x, y, cells.shape[1], cells.shape[0])
    old, new = out[ix] != 0, cells != 0
    out[ix] = np.where({"copy": new, "or": old | new, "xor": old ^ new}[mode], 255, 0)
    return out


def np_view_counts(board, x, y, w, h, scale):
    """Live cells per scale x scale block of the w x h viewport at (x, y) of a 0/255 torus board."""
    win = np.roll(board != 0, (-y, -x), (0, 1))[:h * scale, :w * scale]
    return win.reshape(h, scale, w, scale).sum(axis=(1, 3)).astype(np.uint32)


def np_grey(counts, scale):
    c = counts.astype(np.uint64)
    return ((c * 255 + scale * scale - 1) // (scale * scale)).astype(np.uint8)


def np_rule_step(cells, rule):
    """One generation of a 0/1 torus board under (birth, survive) masks."""
    birth, survive = rule
    c = cells.astype(np.int64)
    n = sum(np.roll(np.roll(c, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    return np.where(cells == 1, (survive >> n) & 1, (birth >> n) & 1).astype(np.uint8)


def flips_of(a, b):
    ys, xs = np.nonzero(a != b)
    return np.stack([xs, ys], 1).astype(np.int32)


def rects(W, H):
    """(x, y, w, h): the full board; the full size at (5, 3), wrapping both ways; 1 x 1; 33 wide at
    x = 31 (one bit over a word boundary on each side); negative origin, odd size; the last column
    and the first."""
    return [(0, 0, W, H), (5, 3, W, H), (W // 2, H // 3, 1, 1), (31, 2, min(33, W), min(5, H)),
            (-5, -3, min(7, W), min(9, H)), (W - 1, H - 2, 2, 3)]


def stamp_cells(w, h, seed):
    return np.where(np.random.default_rng(seed).random((h, w)) < 0.5, 255, 0).astype(np.uint8)


def check_rects(e, board):
    H, W = board.shape
    for (x, y, w, h) in rects(W, H):
        got = e.store_rect(x, y, w, h)
        assert got.shape == (h, w) and np.array_equal(got, np_rect(board, x, y, w, h)), (x, y, w, h)


def stamp_rects(e, board, modes):
    """Every rectangle of rects() stamped with random cells, the mode cycling through `modes`; the
    whole board is compared after each."""
    H, W = board.shape
    ref = board.copy()
    for i, (x, y, w, h) in enumerate(rects(W, H)):
        mode, cells = modes[i % len(modes)], stamp_cells(w, h, 7 * i + W)
        e.load_rect(x, y, cells, mode)
        ref = np_edit(ref, x, y, cells, mode)
        assert np.array_equal(e.store(), ref), (mode, x, y, w, h)
    return ref


# ---------------------------------------------------------------- 1. store_rect geometry
@pytest.mark.parametrize("W,H", BOARDS)
def test_store_rect_geometry(golhip, W, H):
    board = random_board(W, H)
    with golhip.Engine(W, H, k=8) as e:
        e.load(board)
        check_rects(e, board)
        assert np.array_equal(e.store(), board)


# ---------------------------------------------------------------- 2. load_rect modes
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", BOARDS)
def test_load_rect_modes(golhip, oracle, W, H, mode):
    """copy / or / xor into every rectangle; on the replicated 16x16 and 48x37 boards the stamped
    board is then stepped: a replica the stamp missed is a wrong neighbour across x = width."""
    board = random_board(W, H)
    with golhip.Engine(W, H, k=8) as e:
        e.load(board)
        e.step(3)
        ref = stamp_rects(e, oracle.packed_run(board, 3)[0], [mode])
        assert e.turn == 3
        if (W, H) in ((16, 16), (48, 37)):
            counts = e.step(23, counts=True)
            want, want_counts = oracle.packed_run(ref, 23)
            assert np.array_equal(counts.astype(np.int64), want_counts)
            assert np.array_equal(e.store(), want)


# ---------------------------------------------------------------- 3. invalidation
@pytest.mark.parametrize("track", [False, True])
def test_load_rect_invalidates_flips_and_keeps_the_turn(golhip, oracle, track):
    W, H = 200, 96
    board = random_board(W, H)
    n = 5 if track else 1  # without tracking, flips need a last launch of one generation
    with golhip.Engine(W, H, k=8) as e:
        e.track_flips(track)
        e.load(board)
        e.step(n)
        before = oracle.packed_run(board, n - 1)[0] if n > 1 else board
        now = oracle.packed_run(board, n)[0]
        assert np.array_equal(e.flips(), flips_of(before, now))
        cells = stamp_cells(40, 30, 5)
        e.load_rect(-7, 80, cells, "xor")
        with pytest.raises(golhip.GolHipError) as ex:
            e.flips()
        assert ex.value.code == golhip.ERR_STATE
        assert e.turn == n
        stamped = np_edit(now, -7, 80, cells, "xor")
        assert np.array_equal(e.store(), stamped)
        e.step(n)
        before = oracle.packed_run(stamped, n - 1)[0] if n > 1 else stamped
        after = oracle.packed_run(stamped, n)[0]
        assert np.array_equal(e.flips(), flips_of(before, after))
        assert e.turn == 2 * n and np.array_equal(e.store(), after)


def test_stamp_into_a_skipped_slab(golhip, oracle):
    """Stable-slab skipping on (the smallest eligible shape of tests/test_gpu_activity.py, 600 wide:
    16 horizontal replicas): a field of blocks settles until slabs are skipped, then a glider is
    dropped in.  Flags from before the stamp must not be trusted: board and counts equal the oracle.
    (This board also caught a race in the skip path itself: 3 cells of the glider's generation 32
    left in the final board, every count right -- slower waves read the slab's `same` flag after
    wave 0 had set it and skipped their copy.)"""
    W, H = 600, 1000
    field = np.zeros((H, W), np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            field[dy::16, dx::16] = 255
    with golhip.Engine(W, H, k=16) as e:
        e.set_activity(1)
        e.load(field)
        e.step(64, counts=True)
        e.step(64, counts=True)
        skipped = e.activity_stats()[1]
        assert skipped > 0
        assert np.array_equal(e.store(), field)  # still lifes
        e.place(GLIDER, 293, 501)
        assert e.turn == 128
        stamped = np_edit(field, 293, 501, GLIDER, "or")
        counts = e.step(64, counts=True)
        want, want_counts = oracle.packed_run(stamped, 64)
        assert np.array_equal(counts.astype(np.int64), want_counts)
        assert np.array_equal(e.store(), want)
        assert e.activity_stats()[1] > skipped  # and skipping went on around the glider


def test_stamp_between_graph_replays(golhip, oracle):
    """Captured graphs stay valid across a stamp: the same buffers, the same parity."""
    W = H = 512
    board = random_board(W, H)
    cells = stamp_cells(40, 40, 11)
    with golhip.Engine(W, H, k=16) as e:
        e.set_graphs(1)
        e.load(board)
        e.step(256)
        e.load_rect(-7, 500, cells, "xor")
        e.step(256)
        got = e.store()
        assert e.turn == 512
    mid = np_edit(oracle.packed_run(board, 256)[0], -7, 500, cells, "xor")
    assert np.array_equal(got, oracle.packed_run(mid, 256)[0])


# ---------------------------------------------------------------- 4. the viewport
def fill_board(W, H, fill):
    if fill == "random":
        return random_board(W, H)
    if fill == "full":
        return np.full((H, W), 255, np.uint8)
    b = np.zeros((H, W), np.uint8)
    b[(2 * H) // 3, W // 3] = 255
    return b


def check_view(e, board, x, y, w, h, scale):
    want = np_view_counts(board, x, y, w, h, scale)
    got = e.view_counts(x, y, w, h, scale)
    assert got.dtype == np.uint32 and got.shape == (h, w)
    assert np.array_equal(got, want), (x, y, w, h, scale, np.argwhere(got != want)[:5])
    assert np.array_equal(e.view(x, y, w, h, scale), np_grey(want, scale)), (x, y, w, h, scale)
    return want


@pytest.mark.parametrize("fill", ["random", "one", "full"])
@pytest.mark.parametrize("W,H,scales,window", [
    (256, 256, [1, 2, 4, 8, 16, 32, 64, 128], None),
    (2048, 1024, [64, 256, 512, 1024], None),  # scale >= 128: one pixel over 2, 4, 8 lanes
    (16, 16, [1, 2, 4], None),           # replicated torus, scale < 32
    (48, 37, [1, 2, 4], (40, 30, 9, 9)),  # a 9 x 9 window that wraps both ways
])
def test_view_counts_and_grey(golhip, W, H, scales, window, fill):
    """The largest window that fits at every scale, from an aligned, an unaligned and a wrapping
    origin: counts and grey against numpy, on a random board, a board with one live cell (grey 1 in
    exactly one pixel once a block has 255 cells or more) and an all-live board (255 everywhere)."""
    board = fill_board(W, H, fill)
    with golhip.Engine(W, H, k=8) as e:
        e.load(board)
        for scale in scales:
            w, h = W // scale, H // scale
            for (x, y) in ((0, 0), (37, 5), (-(scale // 2), -3)):
                counts = check_view(e, board, x, y, w, h, scale)
                if fill == "full":
                    assert (counts == scale * scale).all()
                    assert (e.view(x, y, w, h, scale) == 255).all()
                if fill == "one" and (w * scale, h * scale) == (W, H):
                    grey = e.view(x, y, w, h, scale)
                    assert counts.sum() == 1 and np.count_nonzero(grey) == 1
                    assert grey.max() == -(-255 // (scale * scale))  # 1 from scale 16 on
            if window:
                check_view(e, board, *window, scale)
        x, y, w, h = window or (37, 5, W, H)
        assert np.array_equal(e.view(x, y, w, h, 1), e.store_rect(x, y, w, h))
        assert np.array_equal(e.store(), board)


# ---------------------------------------------------------------- 5. strips
@pytest.mark.parametrize("stage", [0, 4096])
@pytest.mark.parametrize("W,H", [(48, 37), (2048, 40)])
def test_strips_serve_their_rows(golhip, oracle, monkeypatch, W, H, stage):
    """A handle of 3 strips (13 / 12 / 12 and 13 / 13 / 14 rows): rectangles that span every strip
    and wrap the rows, stamps in every mode followed by steps, and a scale-8 viewport whose blocks
    straddle the strip boundaries (partial counts summed).  stage = 4096 shrinks the transfer stage
    so every call runs in many chunks."""
    if stage:
        monkeypatch.setenv("GOLHIP_STAGE_BYTES", str(stage))
    board = random_board(W, H)
    with golhip.Engine(W, H, k=8, strips=3) as e:
        assert e.info.nshards == 3
        e.load(board)
        check_rects(e, board)
        ref = stamp_rects(e, board, MODES)
        check_rects(e, ref)
        w, h = W // 8, H // 8
        for (x, y) in ((0, 0), (37, 5), (-3, H - 10)):
            check_view(e, ref, x, y, w, h, 8)
            check_view(e, ref, x, y, min(w, 5), h, 1)
            check_view(e, ref, x, y, W, 3, 1)  # wider than a small stage: chunks of pixel columns
        counts = e.step(23, counts=True)
        want, want_counts = oracle.packed_run(ref, 23)
        assert np.array_equal(counts.astype(np.int64), want_counts)
        assert np.array_equal(e.store(), want)


# ---------------------------------------------------------------- 6. the ring of one
def test_ring_of_one(golhip, oracle, monkeypatch):
    """The rank-mode path on one GPU (GOLHIP_RING_SELF: one halo'd strip that holds every row)."""
    monkeypatch.setenv("GOLHIP_RING_SELF", "1")
    W, H = 640, 77
    board = random_board(W, H)
    cells = stamp_cells(100, 50, 3)
    with golhip.Engine(W, H, k=8, rank=0, world_size=1, device=0) as e:
        assert e.info.halo_rows == 8
        e.load(board)
        assert np.array_equal(e.store_rect(-9, 60, 300, 40), np_rect(board, -9, 60, 300, 40))
        e.load_rect(600, 70, cells, "xor")  # wraps the columns and the rows: the halos are stale
        ref = np_edit(board, 600, 70, cells, "xor")
        counts = e.step(23, counts=True)
        want, want_counts = oracle.packed_run(ref, 23)
        assert np.array_equal(counts.astype(np.int64), want_counts)
        assert np.array_equal(e.store(), want)
        check_view(e, want, -5, 70, 40, 4, 16)


# ---------------------------------------------------------------- 7. two ranks
RANK_BOARD = (576, 101)        # 8 replicas; strips of 50 and 51 rows
RANK_RECT = (-6, 90, 200, 60)  # rows 90 .. 149 mod 101: both strips, wrapping
RANK_VIEW = (-6, 90, 100, 24, 4)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, out_dir):
    for p in (str(ROOT / "oracle"), str(PKG)):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import golhip

    dist.init_process_group("gloo", rank=rank, world_size=world)
    W, H = RANK_BOARD
    board = random_board(W, H)
    x, y, w, h = RANK_RECT
    res = {}
    with golhip.Engine(W, H, k=8, rank=rank, world_size=world, device=0,
                       host_comm=golhip.GlooHostComm()) as e:
        y0, rows = e.info.y0, e.info.rows
        e.load(board[y0:y0 + rows])
        res["view"] = e.view_counts(*RANK_VIEW)
        res["rect"] = e.store_rect(x, y, w, h)
        try:
            e.view(*RANK_VIEW)
            res["view_code"] = np.array([0])
        except golhip.GolHipError as err:
            res["view_code"] = np.array([err.code])
        e.load_rect(x, y, stamp_cells(w, h, 17), "xor")
        res["counts"] = e.step(16, counts=True)
        res["strip"] = e.store()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_combine(tmp_path, golhip, oracle):
    """Two rank-mode handles over the host transport, each holding half the rows: the calls are
    not collective, rows a rank does not hold read as dead, so the ranks' counts sum and their
    rectangles OR to the whole; the grey form refuses; a stamp lands on whichever rank holds the row."""
    mp.start_processes(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True,
                       start_method="spawn")
    r = [dict(np.load(tmp_path / f"rank{i}.npz")) for i in range(2)]
    W, H = RANK_BOARD
    board = random_board(W, H)
    x, y, w, h = RANK_RECT
    assert np.array_equal(r[0]["view"] + r[1]["view"], np_view_counts(board, *RANK_VIEW))
    assert r[0]["view"].any() and r[1]["view"].any()
    assert np.array_equal(r[0]["rect"] | r[1]["rect"], np_rect(board, x, y, w, h))
    assert not (r[0]["rect"] & r[1]["rect"]).any()
    assert [int(x["view_code"][0]) for x in r] == [golhip.ERR_STATE] * 2
    stamped = np_edit(board, x, y, stamp_cells(w, h, 17), "xor")
    want, want_counts = oracle.packed_run(stamped, 16)
    for i in range(2):
        assert np.array_equal(r[i]["counts"].astype(np.int64), want_counts), i
    assert np.array_equal(np.concatenate([x["strip"] for x in r]), want)


# ---------------------------------------------------------------- 8. rule independence
def test_another_rule(golhip):
    rule = (0x048, 0x00C)  # B36/S23
    W, H = 128, 64
    board = random_board(W, H)
    cells = stamp_cells(50, 20, 23)
    with golhip.Engine(W, H, k=8, rule="B36/S23") as e:
        assert e.launch_kind(8)[0] == "rule"
        e.load(board)
        e.load_rect(100, 55, cells, "copy")
        ref = np_edit(board, 100, 55, cells, "copy")
        assert np.array_equal(e.store_rect(90, 50, 60, 30), np_rect(ref, 90, 50, 60, 30))
        check_view(e, ref, 3, 3, 15, 7, 8)
        counts = e.step(23, counts=True)
        gen, want_counts = (ref != 0).astype(np.uint8), []
        for _ in range(23):
            gen = np_rule_step(gen, rule)
            want_counts.append(int(gen.sum()))
        assert counts.astype(np.int64).tolist() == want_counts
        assert np.array_equal(e.store(), gen * 255)


# ---------------------------------------------------------------- 9. arguments
def test_bad_arguments_leave_the_board_alone(golhip):
    W = H = 64
    board = random_board(W, H)
    cells = stamp_cells(8, 8, 1)
    with golhip.Engine(W, H, k=8) as e:
        e.load(board)

        def refused(call, *names):
            with pytest.raises(golhip.GolHipError) as ex:
                call()
            assert ex.value.code == golhip.ERR_ARG, ex.value
            assert all(n in str(ex.value) for n in names), ex.value

        refused(lambda: e.store_rect(0, 0, 0, 8), "w 0")
        refused(lambda: e.store_rect(0, 0, W + 1, 8), f"w {W + 1}")
        refused(lambda: e.store_rect(0, 0, 8, H + 1), f"hgt {H + 1}")
        refused(lambda: e.load_rect(0, 0, np.zeros((8, W + 1), np.uint8)), f"w {W + 1}")
        refused(lambda: e.view_counts(0, 0, 0, 8, 2), "w 0")
        for scale in (3, 0, 2048, -4):
            refused(lambda: e.view_counts(0, 0, 8, 8, scale), f"scale {scale}")
            refused(lambda: e.view(0, 0, 8, 8, scale), f"scale {scale}")
        refused(lambda: e.view_counts(0, 0, 33, 8, 2), "33", "width")
        refused(lambda: e.view(0, 0, 8, 17, 4), "17", "height")
        refused(lambda: e.load_rect(0, 0, cells, 3), "mode 3")
        refused(lambda: e.load_rect(0, 0, cells, -1), "mode -1")
        # row_stride < w and null buffers, through the raw calls
        L, buf = e._L, np.zeros((8, 8), np.uint8)
        assert L.golhip_store_rect(e._h, 0, 0, 8, 8, buf.ctypes.data, 4) == golhip.ERR_ARG
        assert b"row_stride 4" in L.golhip_last_error(e._h)
        assert L.golhip_load_rect(e._h, 0, 0, 8, 8, buf.ctypes.data, 7, 0) == golhip.ERR_ARG
        assert L.golhip_view(e._h, 0, 0, 8, 8, 2, buf.ctypes.data, 7) == golhip.ERR_ARG
        assert L.golhip_store_rect(e._h, 0, 0, 8, 8, None, 8) == golhip.ERR_ARG
        assert L.golhip_load_rect(e._h, 0, 0, 8, 8, None, 8, 0) == golhip.ERR_ARG
        assert L.golhip_view_counts(e._h, 0, 0, 8, 8, 2, None) == golhip.ERR_ARG
        assert np.array_equal(e.store(), board)
        e.step(1)
        e.flips()  # a refused load_rect invalidated nothing


# ---------------------------------------------------------------- 10. the CLI
def test_gol_view_writes_the_viewport(tmp_path, oracle):
    """gol -view on the reference's 64x64 image: out/64x64x100-view.pgm is the 16 x 16 grey viewport
    of the reference's own 64x64x100 check image; the full-size PGM is unchanged."""
    out = tmp_path / "out"
    p = subprocess.run([str(PKG / "lib" / "gol"), "-w", "64", "-h", "64", "-turns", "100", "-view", "8,8,16,16,2",
                        "-images", str(REF / "images"), "-out", str(out)], cwd=REF, stdin=subprocess.DEVNULL,
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    check = REF / "check" / "images" / "64x64x100.pgm"
    assert (out / "64x64x100.pgm").read_bytes() == check.read_bytes()
    raw = (out / "64x64x100-view.pgm").read_bytes()
    assert raw.startswith(b"P5")
    vw, vh, view = oracle.read_pgm(out / "64x64x100-view.pgm")
    assert (vw, vh) == (16, 16) and view.shape == (16, 16)
    _, _, board = oracle.read_pgm(check)
    assert np.array_equal(view, np_grey(np_view_counts(board, 8, 8, 16, 16, 2), 2))
    assert "File 64x64x100-view output complete" in p.stdout
