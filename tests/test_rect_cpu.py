"""Windowed board access without a GPU: the four symbols (golhip_store_rect, golhip_load_rect,
golhip_view_counts, golhip_view) are exported and bound, the numpy reference the GPU tests compare
against (tests/test_gpu_rect.py holds the same few lines) is pinned on hand-checked cases, and
`gol -view` refuses a bad viewport before any engine exists.

Reference roles: sdl/loop.go (the window that shows the world), gol/distributor.go:93-103 (the `s`
key's PGM of the whole world)."""
import re
import subprocess

import numpy as np

from conftest import PKG, REF, ROOT

RECT_FUNCTIONS = ["golhip_store_rect", "golhip_load_rect", "golhip_view_counts", "golhip_view"]


def np_view_counts(board, x, y, w, h, scale):
    """Live cells per scale x scale block of the w x h viewport at (x, y) of a 0/255 torus board."""
    win = np.roll(board != 0, (-y, -x), (0, 1))[:h * scale, :w * scale]
    return win.reshape(h, scale, w, scale).sum(axis=(1, 3)).astype(np.uint32)


def np_grey(counts, scale):
    c = counts.astype(np.uint64)
    return ((c * 255 + scale * scale - 1) // (scale * scale)).astype(np.uint8)


def test_library_exports_the_rect_functions(golhip):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / "lib" / "libgolhip.so")], text=True)
    exported = set(re.findall(r" T (golhip_\w+)", out))
    assert not [f for f in RECT_FUNCTIONS if f not in exported]
    header = (ROOT / "include" / "golhip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*(golhip_\w+)\s*\(", header, re.M))
    assert set(RECT_FUNCTIONS) <= declared
    assert declared == set(golhip.EXPORTS)
    lib = golhip.load_library()
    for f in RECT_FUNCTIONS:
        assert getattr(lib, f).argtypes is not None
    assert lib.golhip_version() >= 104
    assert (golhip.RECT_COPY, golhip.RECT_OR, golhip.RECT_XOR) == (0, 1, 2)
    for name, value in (("COPY", 0), ("OR", 1), ("XOR", 2)):
        assert re.search(rf"#define GOLHIP_RECT_{name} {value}\b", header)


def test_reference_view_is_pinned():
    rng = np.random.default_rng(1)
    board = np.where(rng.random((32, 48)) < 0.5, 255, 0).astype(np.uint8)
    # scale 1: the cells themselves, 0 / 255, with the window wrapping in both directions
    c1 = np_view_counts(board, 40, 30, 9, 9, 1)
    want = board[np.ix_((np.arange(9) + 30) % 32, (np.arange(9) + 40) % 48)]
    assert np.array_equal(np_grey(c1, 1), want)
    assert set(np.unique(np_grey(np_view_counts(board, 0, 0, 48, 32, 1), 1))) == {0, 255}
    # one live cell in a 16 x 16 block: count 1, grey ceil(255 / 256) = 1, everything else 0
    one = np.zeros((64, 64), np.uint8)
    one[37, 21] = 255
    c16 = np_view_counts(one, 0, 0, 4, 4, 16)
    assert c16.sum() == 1 and c16[2, 1] == 1
    g16 = np_grey(c16, 16)
    assert g16[2, 1] == 1 and np.count_nonzero(g16) == 1
    # the same cell seen through a window that starts at negative coordinates (wraps)
    assert np_view_counts(one, -16, -16, 4, 4, 16)[3, 2] == 1
    # a full block: count scale^2, grey 255
    full = np.full((64, 64), 255, np.uint8)
    for scale in (1, 2, 16, 64):
        c = np_view_counts(full, 5, 3, 64 // scale, 64 // scale, scale)
        assert (c == scale * scale).all() and (np_grey(c, scale) == 255).all()
    # half the cells of a 2 x 2 block: count 2, grey ceil(510 / 4) = 128
    half = np.zeros((4, 4), np.uint8)
    half[0, 0] = half[1, 1] = 255
    c2 = np_view_counts(half, 0, 0, 2, 2, 2)
    assert c2.tolist() == [[2, 0], [0, 0]] and np_grey(c2, 2).tolist() == [[128, 0], [0, 0]]
    # counts up to 1024^2 * 255 do not overflow
    assert np_grey(np.array([[1024 * 1024]], np.uint32), 1024).tolist() == [[255]]


def run_gol(*args):
    return subprocess.run([str(PKG / "lib" / "gol"), *args, "-images", str(REF / "images")], cwd=REF,
                          stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)


def test_gol_refuses_a_bad_view_before_creating_an_engine(tmp_path):
    """A malformed viewport, and one the board cannot satisfy, end `gol` with a non-zero status and
    a message naming the spec -- before the engine is created, so also on a machine without a GPU."""
    for args, spec in ((["-view", "1,2,3"], "1,2,3"),
                       (["-w", "64", "-h", "64", "-view", "0,0,64,64,2"], "0,0,64,64,2"),
                       (["-w", "64", "-h", "64", "-view", "0,0,8,8,3"], "0,0,8,8,3"),
                       (["-w", "64", "-h", "64", "-view", "0,0,0,8,2"], "0,0,0,8,2"),
                       (["-w", "64", "-h", "64", "-view", "0,0,8,8,2x"], "0,0,8,8,2x")):
        p = run_gol(*args, "-turns", "1", "-out", str(tmp_path / "out"))
        assert p.returncode != 0, (args, p.stdout, p.stderr)
        assert spec in p.stderr, (args, p.stderr)
        assert not (tmp_path / "out").exists()
