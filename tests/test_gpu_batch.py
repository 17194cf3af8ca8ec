"""golhip.Batch on the GPU: many independent small tori advanced by one gol_batch launch (one
workgroup per board), the per-board per-turn population history and the on-device settle turn,
each checked per board against the CPU oracle.

Reference role: the reference runs one world per broker (broker/broker.go:157-180); a batch is
what a soup search or a seed sweep runs instead of one Engine per board."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

SHAPES = [(512, 512), (512, 256), (256, 128), (128, 64), (512, 32), (64, 16), (16, 16), (32, 8), (128, 4)]
CALLS = (1, 2, 3, 37, 130)  # the 4-generation groups, the tail loop, odd drift


def random_boards(n, w, h, seed, density=0.37):
    return (np.random.default_rng(seed).random((n, h, w)) < density).astype(np.uint8) * 255


@pytest.mark.parametrize("w,h", SHAPES)
def test_every_shape_matches_the_oracle(golhip, oracle, w, h):
    """5 distinct boards per shape (board 1 all dead, board 3 all alive): every history count of
    every call, the boards after every call and alive_counts() equal the oracle's, board by board."""
    boards = random_boards(5, w, h, w * 7 + h)
    boards[1] = 0
    boards[3] = 255
    with golhip.Batch(w, h, 5) as b:
        b.load(boards)
        assert b.turn == 0
        assert np.array_equal(b.store(), boards)
        assert np.array_equal(b.alive_counts(), (boards != 0).sum(axis=(1, 2)))
        ref = [boards[i].copy() for i in range(5)]
        total = 0
        for n in CALLS:
            hist = b.step(n, history=True)
            total += n
            assert hist.shape == (5, n) and hist.dtype == np.uint32
            assert b.turn == total
            got = b.store()
            alive = b.alive_counts()
            for i in range(5):
                ref[i], counts = oracle.packed_run(ref[i], n, threads=1)
                assert np.array_equal(hist[i].astype(np.int64), counts), (i, n)
                assert np.array_equal(got[i], ref[i]), (i, n)
                assert int(alive[i]) == int(counts[-1]), (i, n)
        assert b.step(0, history=True).shape == (5, 0) and b.turn == total
        if (w, h) == (64, 16):  # a padded row_stride and board_stride, part of the batch
            big = np.full((2, h + 3, w + 5), 7, np.uint8)
            out = b.store(first=2, n=2, out=big[:, :h, :w])
            assert np.array_equal(out[0], ref[2]) and np.array_equal(out[1], ref[3])
            assert (big[:, h:, :] == 7).all() and (big[:, :, w:] == 7).all()
            # a partial load through padded strides lands on the right boards (and resets the turn)
            src = np.zeros((2, h + 1, w + 3), np.uint8)
            src[:, :h, :w] = random_boards(2, w, h, 99)
            b.load(src[:, :h, :w], first=3)
            assert b.turn == 0
            got = b.store()
            assert np.array_equal(got[3:], src[:, :h, :w]) and np.array_equal(got[:3], np.stack(ref[:3]))


def test_more_boards_than_are_resident(golhip, oracle):
    """4099 boards of 128 x 64 from init_random(seed0=11): every board and every count of 40 turns
    against oracle.init_random + packed_run_words; one board also against a single Engine(128, 64)
    from the same seed (the initial words -- init_random parity --, the final words, the counts)."""
    n, w, h, turns, k = 4099, 128, 64, 40, 2077
    with golhip.Batch(w, h, n) as b:
        b.init_random(seed0=11)
        first = b.store(first=k, n=1)[0]
        hist = b.step(turns, history=True)
        got = b.store()
        alive = b.alive_counts()
    got_bits = np.packbits(got != 0, axis=2, bitorder="little")  # (n, h, w / 8)
    for i in range(n):
        words = oracle.init_random(w, h, seed=11 + i)
        if i == k:
            assert np.array_equal(first, oracle.unpack(words, w))
        counts = oracle.packed_run_words(words, turns, threads=1)
        assert np.array_equal(hist[i].astype(np.int64), counts), i
        assert np.array_equal(got_bits[i], words.view(np.uint8).reshape(h, w // 8)), i
    assert np.array_equal(alive, hist[:, -1])
    with golhip.Engine(w, h, k=16) as e:
        e.init_random(11 + k)
        assert np.array_equal(e.store(), first)
        c = e.step(turns, counts=True)
        assert np.array_equal(c.astype(np.uint32), hist[k])
        assert np.array_equal(e.store(), got[k])


def test_seeds_array_and_density(golhip, oracle):
    """init_random(seeds=...) at a density other than one half: board i is the single engine's board
    of seeds[i]."""
    seeds = np.array([5, 5, 2 ** 63 + 9, 0, 77], dtype=np.uint64)
    q = int(0.3 * 2 ** 32)
    with golhip.Batch(64, 64, 5) as b:
        b.init_random(seeds=seeds, density_q32=q)
        got = b.store()
    for i, s in enumerate(seeds):
        assert np.array_equal(got[i], oracle.unpack(oracle.init_random(64, 64, seed=int(s), density_q32=q), 64)), i


CHILD = """
import sys
sys.path.insert(0, {pkg!r})
import numpy as np
import golhip
boards = np.load({inp!r})
with golhip.Batch(64, 16, boards.shape[0]) as b:
    b.load(boards)
    b.track_settle()
    h1 = b.step(50, history=True)
    mid = b.store()
    h2 = b.step(13, history=True)
    np.savez({out!r}, h1=h1, h2=h2, mid=mid, end=b.store(), alive=b.alive_counts(), settled=b.settled())
"""


def test_history_chunking_with_a_small_stage(golhip, oracle, tmp_path):
    """A fresh process whose transfer stage is 256 bytes (GOLHIP_STAGE_BYTES): 7 boards of 64 x 16
    load and store in 4-row chunks and a 50-turn history call runs 6 launches of at most 9
    generations.  Everything equals the unshrunk run in this process, and the oracle."""
    boards = random_boards(7, 64, 16, 3)
    np.save(tmp_path / "in.npy", boards)
    code = CHILD.format(pkg=str(PKG), inp=str(tmp_path / "in.npy"), out=str(tmp_path / "out.npz"))
    env = dict(os.environ, GOLHIP_STAGE_BYTES="256")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, "-c", code], env=env, check=True, timeout=120)
    small = np.load(tmp_path / "out.npz")
    with golhip.Batch(64, 16, 7) as b:
        b.load(boards)
        b.track_settle()
        h1 = b.step(50, history=True)
        mid = b.store()
        h2 = b.step(13, history=True)
        end, alive, settled = b.store(), b.alive_counts(), b.settled()
    for name, want in (("h1", h1), ("h2", h2), ("mid", mid), ("end", end), ("alive", alive), ("settled", settled)):
        assert np.array_equal(small[name], want), name
    for i in range(7):
        r50, c50 = oracle.packed_run(boards[i], 50, threads=1)
        r63, c13 = oracle.packed_run(r50, 13, threads=1)
        assert np.array_equal(h1[i].astype(np.int64), c50) and np.array_equal(h2[i].astype(np.int64), c13)
        assert np.array_equal(mid[i], r50) and np.array_equal(end[i], r63)


# ------------------------------------------------------------------------------- settling
SOUPS, SOUP_TURNS = 24, 6000


@pytest.fixture(scope="module")
def soup_settle_turns(oracle):
    """Per seed 0..23 of a 64 x 64 half-density soup: the smallest turn t >= 2 with
    board(t) == board(t - 2), from the CPU oracle stepped one generation at a time (-1: not within
    SOUP_TURNS)."""
    out = []
    for seed in range(SOUPS):
        cur = oracle.init_random(64, 64, seed=seed)
        before, before2 = cur.copy(), None  # board(t - 1), board(t - 2)
        settled = -1
        for t in range(1, SOUP_TURNS + 1):
            oracle.packed_run_words(cur, 1, threads=1)
            if before2 is not None and np.array_equal(cur, before2):
                settled = t
                break
            before2, before = before, cur.copy()
        out.append(settled)
    return np.array(out, dtype=np.int64)


def known_by(expected, turn):
    return np.where((expected >= 0) & (expected <= turn), expected, -1)


def test_soups_settle_when_the_oracle_says(golhip, soup_settle_turns):
    """24 soups, tracking on: settled() after 2000 turns and after 4000 more equals the oracle's
    settle turns (-1 where not reached yet: seeds 7, 9, 12, 16, 18, 19 at 2000; seed 7 settles past
    the 4096-generation launch bound).  A second batch stepped as 1, 1, 2, 1996, 4000 gives the same
    answers, and tracking changes neither the history nor the boards."""
    exp = soup_settle_turns
    assert (exp >= 2).all() and exp.min() == exp[0] == 308 and exp.max() == exp[7] == 5502
    assert sorted(np.nonzero(exp > 2000)[0]) == [7, 9, 12, 16, 18, 19]
    with golhip.Batch(64, 64, SOUPS) as b, golhip.Batch(64, 64, SOUPS) as cut, golhip.Batch(64, 64, SOUPS) as plain:
        for x in (b, cut, plain):
            x.init_random(seed0=0)
        b.track_settle()
        cut.track_settle()
        assert (b.settled() == -1).all()
        h_tracked = b.step(2000, history=True)
        s2000 = b.settled()
        assert np.array_equal(s2000, known_by(exp, 2000)), (s2000, exp)
        b.step(4000)
        s6000 = b.settled()
        assert np.array_equal(s6000, exp), (s6000, exp)
        assert b.turn == 6000
        got = []
        for n in (1, 1, 2, 1996, 4000):
            cut.step(n)
            got.append(cut.settled())
        assert (got[0] == -1).all() and (got[1] == -1).all() and (got[2] == -1).all()
        assert np.array_equal(got[3], s2000) and np.array_equal(got[4], s6000)
        h_plain = plain.step(2000, history=True)
        plain.step(4000)
        assert np.array_equal(h_tracked, h_plain)
        assert np.array_equal(b.store(), plain.store()) and np.array_equal(cut.store(), plain.store())
        with pytest.raises(golhip.GolHipError) as ei:
            plain.settled()  # tracking is off
        assert ei.value.code == golhip.ERR_STATE


def test_hand_cases_settle(golhip):
    """A block and a blinker (and both with an empty board between) settle at turn 2, the earliest
    turn there is; a lone glider on the torus never does."""
    boards = np.zeros((4, 64, 64), np.uint8)
    boards[0, 10:12, 20:22] = 255  # block
    boards[1, 30, 40:43] = 255     # blinker
    boards[3, 0, 1] = boards[3, 1, 2] = boards[3, 2, 0] = boards[3, 2, 1] = boards[3, 2, 2] = 255  # glider
    for cuts in ((300,), (1, 1, 1, 297)):
        with golhip.Batch(64, 64, 4) as b:
            b.load(boards)
            b.track_settle()
            for n in cuts:
                b.step(n)
                want = [2, 2, 2, -1] if b.turn >= 2 else [-1] * 4
                assert b.settled().tolist() == want, (cuts, b.turn)
            assert b.alive_counts().tolist() == [4, 3, 0, 5]


# ------------------------------------------------------------------------------- contract
def test_contract(golhip):
    for args, value in (((48, 48, 4), "48"), ((64, 100, 4), "100"), ((64, 64, 0), "0"), ((1024, 64, 1), "1024")):
        with pytest.raises(golhip.GolHipError) as ei:
            golhip.Batch(*args)
        assert ei.value.code == golhip.ERR_ARG and value in str(ei.value), (args, str(ei.value))
    with golhip.Batch(16, 16, 3) as b:
        with pytest.raises(golhip.GolHipError) as ei:
            b.init_random(seed0=1)
        assert ei.value.code == golhip.ERR_ARG
    with golhip.Batch(64, 512, 2) as b:  # 512 rows: the single engine only picks gol_board up to 256
        b.init_random(seed0=4)
        b.step(3)
        assert b.turn == 3
        with pytest.raises(golhip.GolHipError) as ei:
            b.track_settle()
        assert ei.value.code == golhip.ERR_STATE
        b.track_settle(False)
        for bad in ((2, 1), (-1, 1), (0, 3)):  # boards outside the batch
            with pytest.raises(golhip.GolHipError) as ei:
                b.store(first=bad[0], n=bad[1])
            assert ei.value.code == golhip.ERR_ARG
        b.load(np.zeros((1, 512, 64), np.uint8), first=1)  # part of the batch: the turn still resets
        assert b.turn == 0
        b.track_settle()
        b.step(2)
        assert b.settled()[1] == 2
        b.init_random(seed0=4)
        assert b.turn == 0 and (b.settled() == -1).all()
