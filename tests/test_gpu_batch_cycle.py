"""The exact soup search on golhip.Batch (golhip_batch_search_exact, the kernel gol_batch_cycle of
csrc/batch_cycle.hpp): search() plus cycle_start, the least t >= 0 with board(t + period) ==
board(t), -1 for a soup without a repeat within max_turns.

The reference is a numpy brute force (np_cycles): every soup's cells -- from the existing path,
init_random(seeds) then store(), with the cells outside a soup box cleared -- are stepped turn by
turn, every state is hashed, and the first state seen twice gives (cycle_start, period).  Every
comparison is exact: cycle_start for the soups whose record has a repeat, -1 for the others, and the
records byte for byte against Batch.search's."""
import hashlib

import numpy as np
import pytest

from test_gpu_batch_period import HIGHLIFE, LIFE, STROBE, TABLE_RULE, np_step_boards, soups
from test_gpu_batch_plane import box_mask, np_step_plane
from test_gpu_batch_search import HALF, soup_cells

pytestmark = pytest.mark.gpu


def np_cycles(cells, rules, max_turns, plane=False):
    """(cycle_start, period) int64 arrays of an (n, h, w) stack of 0/1 boards, board i under rules[i]
    (a single pair: every board under it), by brute force: the first state of board(0..max_turns)
    seen twice, at turns a < b, gives cycle_start = a and period = b - a; (-1, -1) if there is none.
    On a plane whose rules have no B0 only the window around the live cells is stepped: a cell two
    or more away from every live cell stays dead."""
    cur = np.ascontiguousarray(cells, dtype=np.uint8)
    n, h, w = cur.shape
    pairs = np.asarray(rules, dtype=np.int32).reshape(-1, 2)
    windowed = plane and not (pairs[:, 0] & 1).any()
    start = np.full(n, -1, dtype=np.int64)
    period = np.full(n, -1, dtype=np.int64)
    seen = [{} for _ in range(n)]
    open_ = set(range(n))
    for t in range(max_turns + 1):
        packed = np.packbits(cur.reshape(n, -1), axis=1)
        for i in sorted(open_):
            key = hashlib.blake2b(packed[i].tobytes(), digest_size=16).digest()
            if key in seen[i]:
                start[i], period[i] = seen[i][key], t - seen[i][key]
                open_.discard(i)
            else:
                seen[i][key] = t
        if not open_:
            break
        if not plane:
            cur = np_step_boards(cur, rules)
        elif not windowed:
            cur = np_step_plane(cur, rules)
        else:
            ys, xs = np.nonzero(cur.any(axis=(0, 2)))[0], np.nonzero(cur.any(axis=(0, 1)))[0]
            if ys.size:
                y0, y1 = max(int(ys[0]) - 1, 0), min(int(ys[-1]) + 2, h)
                x0, x1 = max(int(xs[0]) - 1, 0), min(int(xs[-1]) + 2, w)
                nxt = np.zeros_like(cur)
                nxt[:, y0:y1, x0:x1] = np_step_plane(cur[:, y0:y1, x0:x1], rules)
                cur = nxt
    return start, period


def boxed_cells(golhip, w, h, seeds, box=None, density=HALF):
    cells = soup_cells(golhip, w, h, seeds, density)
    return cells if box is None else cells * box_mask(w, h, box)[None]


def check_exact(golhip, b, cells, seeds, max_turns, rules_of_soups, plane, where="", **search_args):
    """search_exact against search (the records) and the brute force (cycle_start).  Returns (records,
    cycle_start, the floors) for the conditions a test puts on its seeds."""
    want_start, want_period = np_cycles(cells, rules_of_soups, max_turns, plane)
    rec = b.search(len(seeds), seeds=seeds, max_turns=max_turns, **search_args)
    got, start = b.search_exact(len(seeds), seeds=seeds, max_turns=max_turns, **search_args)
    assert got.dtype == golhip.SOUP_DTYPE and start.dtype == np.int64 and start.shape == (len(seeds),)
    assert got.tobytes() == rec.tobytes(), where
    repeated = rec["repeat_turn"] >= 0
    # a repeat Brent's scheme has seen within max_turns is one the brute force has seen
    assert (want_start[repeated] >= 0).all() and np.array_equal(rec["period"][repeated], want_period[repeated]), where
    want = np.where(repeated, want_start, -1)
    bad = np.nonzero(start != want)[0]
    assert bad.size == 0, (where, bad[:8], start[bad[:8]], want[bad[:8]], rec[bad[:8]])
    floor = np.array([golhip.cycle_start_floor(int(r), int(p)) for r, p in zip(rec["repeat_turn"], rec["period"])])
    assert ((floor <= start) & (start <= rec["repeat_turn"] - rec["period"]))[repeated].all(), where
    return rec, start, floor


# ---------------------------------------------------------------- 1. every shape of the table, at width 64
# (height, max_turns, plane with a 16 x 16 box, seeds): (W, R) = (1, 1), (1, 2), (1, 4), (2, 4), (4, 4),
# (8, 4), (16, 4), (16, 8).  The seeds are picked so that the reference meets the conditions below;
# the comparison with the brute force comes first, then the conditions are asserted on the results
# it has confirmed.  On the 64 x 4 torus only a fifth of the random soups repeat within 300 turns
# (the rest circle on: 230 of seeds 0..1023), so no range of consecutive seeds has half its soups
# repeat there: that shape takes the repeating seeds among 0..109, twelve that do not, and seed 383,
# whose cycle starts at its snapshot turn 15.  64 x 8 takes seeds 120..151: seed 141 is of that kind too.
SEEDS_64X4 = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 20, 22, 24, 30, 38, 39, 54, 55, 63, 71, 74, 87,
              100, 109, 383)
SHAPES = [(4, 300, False, SEEDS_64X4), (8, 300, False, range(120, 152)), (16, 600, False, range(32)),
          (32, 1100, False, range(24)), (64, 1100, True, range(16)), (128, 1100, True, range(16)),
          (256, 1100, True, range(16)), (512, 1100, True, range(16))]

_shape_results = {}  # height -> (records, cycle_start, floor), computed once


def shape_results(golhip, h, max_turns, plane, seeds):
    if h not in _shape_results:
        seeds = np.array(seeds, dtype=np.uint64)
        box = (16, 16) if plane else None
        cells = boxed_cells(golhip, 64, h, seeds, box)
        with golhip.Batch(64, h, 1, topology="plane" if plane else "torus", soup_box=box) as b:
            _shape_results[h] = check_exact(golhip, b, cells, seeds, max_turns, LIFE, plane)
    return _shape_results[h]


@pytest.mark.parametrize("h,max_turns,plane,seeds", SHAPES, ids=[f"64x{s[0]}" for s in SHAPES])
def test_every_shape(golhip, h, max_turns, plane, seeds):
    rec, start, floor = shape_results(golhip, h, max_turns, plane, seeds)
    repeated = rec["repeat_turn"] >= 0
    snap = rec["repeat_turn"] - rec["period"]
    # the seeds alone: at least half the soups repeat, and one enters its cycle strictly between
    # turn 0 and its snapshot turn
    assert 2 * int(repeated.sum()) >= len(seeds), rec["repeat_turn"]
    assert (repeated & (start > 0) & (start < snap)).any(), (start, snap)


def test_the_shapes_cover_the_edges(golhip):
    """Somewhere among the shapes above: a soup whose cycle starts exactly at its snapshot turn (> 0),
    and a soup whose record gives no lower bound (a period above half its window: the circling
    gliders of a short torus) although its cycle starts later than turn 0."""
    at_snapshot = no_floor = 0
    for shape in SHAPES[:2]:  # the two shapes whose seeds were picked for it
        rec, start, floor = shape_results(golhip, *shape)
        repeated = rec["repeat_turn"] >= 0
        snap = rec["repeat_turn"] - rec["period"]
        at_snapshot += int((repeated & (start == snap) & (snap > 0)).sum())
        no_floor += int((repeated & (floor == 0) & (start > 0)).sum())
    assert at_snapshot >= 1 and no_floor >= 1, (at_snapshot, no_floor)


def test_512x512_runs_unreplicated(golhip):
    """wd = 16: no lane holds a replica.  Plane, 16 x 16 box, 4 soups, 600 turns."""
    seeds = np.arange(4, dtype=np.uint64)
    cells = boxed_cells(golhip, 512, 512, seeds, (16, 16))
    with golhip.Batch(512, 512, 1, topology="plane", soup_box=(16, 16)) as b:
        rec, start, _ = check_exact(golhip, b, cells, seeds, 600, LIFE, True)
    assert (rec["repeat_turn"] >= 0).any() and (start > 0).any(), (rec, start)


# ---------------------------------------------------------------- 2. rules
@pytest.mark.parametrize("rule,max_turns", [(HIGHLIFE, 600), (TABLE_RULE, 300)], ids=["highlife", "table"])
def test_a_uniform_rule_runs_the_table_form(golhip, rule, max_turns):
    """HighLife's search runs constant-folded and its exact pass in the table form: the results are
    the rule's.  B38/S0236 burns on: no soup repeats, every cycle_start is -1."""
    seeds = np.arange(32, dtype=np.uint64)
    cells = boxed_cells(golhip, 64, 16, seeds)
    with golhip.Batch(64, 16, 2, rule=rule) as b:
        rec, start, _ = check_exact(golhip, b, cells, seeds, max_turns, rule, False)
    if rule == HIGHLIFE:
        assert (start > 0).any() and (start < 0).any(), start
    else:
        assert (start == -1).all(), start


def test_a_b0_rule_strobes(golhip):
    """B03/S23 on an empty board: full, empty, full, ...: (3, 2) with cycle_start 0, on the torus and on
    the plane (where the border cells of the full board die differently: the brute force decides)."""
    seeds = np.arange(2, dtype=np.uint64)
    empty = np.zeros((2, 16, 64), dtype=np.uint8)
    for topology in ("torus", "plane"):
        with golhip.Batch(64, 16, 1, rule=STROBE, topology=topology) as b:
            rec, start, _ = check_exact(golhip, b, empty, seeds, 300, STROBE, topology == "plane", topology,
                                        density_q32=0)
            if topology == "torus":
                assert (rec["repeat_turn"] == 3).all() and (start == 0).all(), (rec, start)
            got, start = b.search_exact(2, density_q32=0, max_turns=2)
            assert (got["repeat_turn"] == -1).all() and (start == -1).all()


def test_one_rule_per_soup(golhip):
    """One seed under 32 rules (B3/S23, HighLife, the table rule, the strobing rule and 28 drawn masks),
    and equal to each rule as the batch's uniform rule."""
    rng = np.random.default_rng(64)
    rules = [LIFE, HIGHLIFE, TABLE_RULE, STROBE] + [tuple(int(v) for v in rng.integers(0, 512, 2)) for _ in range(28)]
    seed, max_turns = 17, 300
    seeds = np.full(32, seed, dtype=np.uint64)
    cells = np.repeat(boxed_cells(golhip, 64, 16, [seed]), 32, axis=0)
    with golhip.Batch(64, 16, 32, rules=[STROBE] * 32) as b:  # the handle's per-board rules are not the soups'
        rec, start, _ = check_exact(golhip, b, cells, seeds, max_turns, rules, False, rules=rules)
        assert len(set(start.tolist())) >= 4, start
        b.set_rules(None)
        for i, rule in enumerate(rules):
            b.set_rule(rule)
            one, s1 = b.search_exact(1, seeds=[seed], max_turns=max_turns)
            assert one[0] == rec[i] and s1[0] == start[i], (i, rule, one[0], s1[0], start[i])


# ---------------------------------------------------------------- 3. topology, box, density
def test_a_torus_with_a_box(golhip):
    seeds = np.arange(100, 116, dtype=np.uint64)
    cells = boxed_cells(golhip, 64, 32, seeds, (12, 10))
    with golhip.Batch(64, 32, 1, soup_box=(12, 10)) as b:
        rec, start, _ = check_exact(golhip, b, cells, seeds, 1100, LIFE, False)
    assert (start > 0).any(), start


def test_a_plane_without_a_box(golhip):
    seeds = np.arange(16, dtype=np.uint64)
    cells = boxed_cells(golhip, 64, 16, seeds)
    with golhip.Batch(64, 16, 1, topology="plane") as b:
        rec, start, _ = check_exact(golhip, b, cells, seeds, 600, LIFE, True)
    assert (start > 0).any(), start


def test_the_sparse_density_path(golhip):
    """Density 0.04: the per-cell seeding path, 256 x 128 (8 torus words, (W, R) = (8, 4))."""
    seeds = np.arange(8, dtype=np.uint64)
    cells = boxed_cells(golhip, 256, 128, seeds, None, 0x0A3D70A3)
    with golhip.Batch(256, 128, 1) as b:
        rec, start, _ = check_exact(golhip, b, cells, seeds, 300, LIFE, False, density_q32=0x0A3D70A3)
    assert (rec["repeat_turn"] >= 0).any(), rec


# ---------------------------------------------------------------- 4. the ends of the run
def test_a_repeat_in_the_last_turns(golhip):
    """max_turns == repeat_turn still finds the repeat and the same cycle_start; one less gives -1."""
    seeds = np.arange(32, dtype=np.uint64)
    cells = boxed_cells(golhip, 64, 16, seeds)
    want_start, _ = np_cycles(cells, LIFE, 600)
    with golhip.Batch(64, 16, 1) as b:
        rec = b.search(32, seeds=seeds, max_turns=600)
        picked = [i for i in np.nonzero(rec["repeat_turn"] > 1)[0]][:6]
        assert len(picked) == 6, rec["repeat_turn"]
        for i in picked:
            r = int(rec["repeat_turn"][i])
            for max_turns, want in ((r, int(want_start[i])), (r + 1, int(want_start[i])), (r - 1, -1)):
                got, start = b.search_exact(1, seeds=seeds[i:i + 1], max_turns=max_turns)
                assert got.tobytes() == b.search(1, seeds=seeds[i:i + 1], max_turns=max_turns).tobytes()
                assert int(start[0]) == want and (got["repeat_turn"][0] >= 0) == (want >= 0), (i, r, max_turns, start)


@pytest.mark.parametrize("w,h", [(64, 4), (64, 64), (512, 512)], ids=["1wave", "4waves", "16waves"])
def test_empty_boards_and_one_turn(golhip, w, h):
    """An empty board is on its cycle at turn 0.  max_turns 1: a soup that is a still life at turn 0
    is (1, 1) with cycle_start 0, every other soup has no repeat and -1."""
    with golhip.Batch(w, h, 1) as b:
        for max_turns in (1, 2, 40, 300):
            got, start = b.search_exact(3, seed0=9, density_q32=0, max_turns=max_turns)
            assert (got["repeat_turn"] == 1).all() and (got["period"] == 1).all() and (start == 0).all()
        got, start = b.search_exact(5, seed0=0, max_turns=1)
        assert got.tobytes() == b.search(5, seed0=0, max_turns=1).tobytes()
        assert np.array_equal(start, np.where(got["repeat_turn"] >= 0, 0, -1)) and (start == -1).any()


# ---------------------------------------------------------------- 5. independence
def test_cycle_start_does_not_depend_on_position_or_nsoups(golhip):
    seeds = np.arange(64, dtype=np.uint64)
    perm = np.random.default_rng(5).permutation(64)
    with golhip.Batch(64, 16, 1) as b:
        rec, start = b.search_exact(64, seed0=0, max_turns=600)
        assert (start > 0).any() and (start < 0).any()
        got, s2 = b.search_exact(64, seeds=seeds[perm], max_turns=600)
        assert np.array_equal(got, rec[perm]) and np.array_equal(s2, start[perm])
        got, s3 = b.search_exact(7, seeds=seeds[20:27], max_turns=600)
        assert np.array_equal(got, rec[20:27]) and np.array_equal(s3, start[20:27])


def test_cycle_start_does_not_depend_on_the_chunks(golhip):
    """65536 + 37 soups of 64 x 4 cross a chunk boundary: the first and the last 512 are those of
    512-soup calls of the same seeds, and the last 64 are the brute force's."""
    n, seed0, max_turns = 65536 + 37, 1 << 40, 64
    with golhip.Batch(64, 4, 2) as b:
        got, start = b.search_exact(n, seed0=seed0, max_turns=max_turns)
        assert got.tobytes() == b.search(n, seed0=seed0, max_turns=max_turns).tobytes()
        first, s_first = b.search_exact(512, seed0=seed0, max_turns=max_turns)
        tail = np.uint64(seed0) + np.arange(n - 512, n, dtype=np.uint64)
        last, s_last = b.search_exact(512, seeds=tail, max_turns=max_turns)
    assert start.shape == (n,)
    assert np.array_equal(got[:512], first) and np.array_equal(start[:512], s_first)
    assert np.array_equal(got[-512:], last) and np.array_equal(start[-512:], s_last)
    assert ((start == -1) == (got["repeat_turn"] < 0)).all()
    assert (start <= got["repeat_turn"] - got["period"]).all()
    cells = boxed_cells(golhip, 64, 4, tail[-64:])
    want_start, _ = np_cycles(cells, LIFE, max_turns)
    repeated = got["repeat_turn"][-64:] >= 0
    assert repeated.any() and np.array_equal(start[-64:], np.where(repeated, want_start, -1))


# ---------------------------------------------------------------- 6. the handle is untouched
def test_search_exact_leaves_the_handle_as_it_was(golhip):
    cells = soups(5, 64, 64, 23)
    rules = [HIGHLIFE, LIFE, TABLE_RULE, LIFE, HIGHLIFE]
    runs = []
    for searched in (False, True):
        with golhip.Batch(64, 64, 5, rules=rules, topology="plane", soup_box=(20, 12)) as b:
            b.load(cells * 255)
            b.track_period()
            b.step(37)
            if searched:
                state = (b.store(), b.turn, b.periods(), b.rules.copy(), b.kernel_form, b.topology, b.soup_box)
                got, start = b.search_exact(40, seed0=3, max_turns=200)
                assert got.shape == (40,) and start.shape == (40,)
                after = (b.store(), b.turn, b.periods(), b.rules.copy(), b.kernel_form, b.topology, b.soup_box)
                assert np.array_equal(after[0], state[0]) and after[1] == state[1] == 37
                assert np.array_equal(after[2][0], state[2][0]) and np.array_equal(after[2][1], state[2][1])
                assert np.array_equal(after[3], state[3]) and after[4:] == state[4:] == (3, "plane", (20, 12))
            b.step(100)
            runs.append((b.store(), b.turn, *b.periods()))
    assert runs[0][1] == runs[1][1] == 137
    for a, c in zip(runs[0], runs[1]):
        assert np.array_equal(a, c)


# ---------------------------------------------------------------- 7. errors
def test_errors(golhip):
    lib = golhip.load_library()
    with golhip.Batch(16, 16, 2) as b:  # init_random's condition
        with pytest.raises(golhip.GolHipError) as ei:
            b.search_exact(4, max_turns=10)
        assert ei.value.code == golhip.ERR_ARG and "width" in str(ei.value)
    cells = soups(2, 64, 16, 3)
    with golhip.Batch(64, 16, 2) as b:
        b.load(cells * 255)
        b.step(5)
        state = (b.store(), b.turn)
        out = np.full(4, 7, dtype=golhip.SOUP_DTYPE)
        starts = np.full(4, 7, dtype=np.int64)
        untouched, untouched_starts = out.copy(), starts.copy()
        good = np.array([8, 8, 8, 8], dtype=np.uint32)
        bad = np.array([8, 8, 0x208, 8], dtype=np.uint32)

        def call(nsoups=4, max_turns=10, birth=None, survive=None, out=out, starts=starts):
            return lib.golhip_batch_search_exact(b._h, nsoups, None, 0, HALF, max_turns,
                                                 None if birth is None else birth.ctypes.data,
                                                 None if survive is None else survive.ctypes.data,
                                                 None if out is None else out.ctypes.data,
                                                 None if starts is None else starts.ctypes.data)

        for kwargs, words in ((dict(max_turns=0), ["max_turns"]), (dict(max_turns=(1 << 20) + 1), ["max_turns"]),
                              (dict(max_turns=-3), ["max_turns"]), (dict(nsoups=-1), ["nsoups"]),
                              (dict(birth=bad, survive=good), ["soup 2", "0x208"]),
                              (dict(birth=good, survive=bad), ["soup 2", "0x208"]),
                              (dict(birth=good), ["birth", "survive"]), (dict(survive=good), ["birth", "survive"]),
                              (dict(out=None), ["out"]), (dict(starts=None), ["cycle_start"])):
            assert call(**kwargs) == golhip.ERR_ARG, kwargs
            why = lib.golhip_batch_last_error(b._h).decode()
            assert all(word in why for word in words), (kwargs, why)
            assert np.array_equal(out, untouched) and np.array_equal(starts, untouched_starts), kwargs
            assert np.array_equal(b.store(), state[0]) and b.turn == state[1], kwargs
        for kwargs in (dict(max_turns=0), dict(max_turns=(1 << 20) + 1), dict(nsoups=-1),
                       dict(rules=[LIFE, (0x208, 8), LIFE, LIFE]), dict(rules=[LIFE] * 3), dict(seeds=[1, 2, 3])):
            with pytest.raises(golhip.GolHipError) as ei:
                b.search_exact(**{"nsoups": 4, "max_turns": 10, **kwargs})
            assert ei.value.code == golhip.ERR_ARG, kwargs
        # no soups: a no-op, whatever the outputs are
        assert call(nsoups=0, out=None, starts=None) == golhip.OK and call(nsoups=0) == golhip.OK
        assert np.array_equal(out, untouched) and np.array_equal(starts, untouched_starts)
        got, start = b.search_exact(0, max_turns=10)
        assert got.shape == (0,) and start.shape == (0,)
        # the handle still works
        assert call(max_turns=300) == golhip.OK and not np.array_equal(out, untouched)
        got, start = b.search_exact(4, max_turns=300)
        assert np.array_equal(out, got) and np.array_equal(starts, start)
        assert np.array_equal(out, b.search(4, max_turns=300))
        assert np.array_equal(b.store(), state[0]) and b.turn == state[1]
        b.step(3)
        assert b.turn == 8
