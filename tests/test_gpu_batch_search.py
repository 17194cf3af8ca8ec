"""The soup search on golhip.Batch (golhip_batch_search, the kernel gol_batch_search of
csrc/batch_search.hpp): a soup is a seed, one workgroup generates its board in registers and runs
it until it repeats or max_turns have run.

Two references, every comparison exact.  The soups themselves come from the existing Batch path:
init_random(seeds) then store().  Their records come from the numpy definition restated in
tests/test_gpu_batch_period.py (np_step_boards, np_periods): repeat_turn and period as periods()
defines them after max_turns turns, stop_turn the documented function of (repeat_turn, max_turns),
restated here (stop_turn_of), and population the alive count after stop_turn turns."""
import numpy as np
import pytest

from test_gpu_batch_period import HIGHLIFE, LIFE, STROBE, TABLE_RULE, np_periods, period_of, soups

pytestmark = pytest.mark.gpu

HALF = 0x80000000
FIELDS = ("repeat_turn", "period", "stop_turn", "population", "reserved")


def f(r):
    """The turn at which a soup that repeats at turn r is retired, max_turns permitting: the kernel
    takes the match masks once per 32 generations and every wave leaves 8 generations later."""
    return 32 * ((r - 1) // 32) + 40


def stop_turn_of(repeat_turn, max_turns):
    return np.array([max_turns if r < 0 else min(max_turns, f(r)) for r in repeat_turn], dtype=np.int64)


def records(repeat_turn, counts, max_turns):
    """The records of soups with these repeat turns (after max_turns turns) and these (n, >= max_turns)
    alive counts per turn."""
    repeat_turn = np.asarray(repeat_turn, dtype=np.int64)
    assert ((repeat_turn == -1) | ((repeat_turn >= 1) & (repeat_turn <= max_turns))).all()
    stop = stop_turn_of(repeat_turn, max_turns)
    assert ((stop >= np.maximum(repeat_turn, 1)) & (stop <= max_turns)).all()
    assert ((repeat_turn < 0) | (stop == max_turns) | (stop - repeat_turn <= 96)).all()
    population = np.asarray(counts)[np.arange(len(stop)), stop - 1].astype(np.int64)
    return {"repeat_turn": repeat_turn, "period": period_of(repeat_turn), "stop_turn": stop,
            "population": population, "reserved": np.zeros(len(stop), dtype=np.int64)}


def np_records(cells, rules, max_turns):
    ref, counts, _ = np_periods(cells, rules, max_turns)
    return records(ref[max_turns], counts, max_turns)


def check(got, want, where=""):
    assert got.dtype.names == FIELDS and got.dtype.itemsize == 32
    assert got.shape == want["repeat_turn"].shape, where
    for name in FIELDS:
        bad = np.nonzero(got[name].astype(np.int64) != want[name])[0]
        assert bad.size == 0, (where, name, bad[:8], got[name][bad[:8]], want[name][bad[:8]])


def soup_cells(golhip, w, h, seeds, density_q32=HALF):
    """The soups as the existing path makes them: init_random(seeds), store()."""
    seeds = np.asarray(seeds, dtype=np.uint64)
    with golhip.Batch(w, h, len(seeds)) as b:
        b.init_random(seeds=seeds, density_q32=density_q32)
        cells = (b.store() != 0).astype(np.uint8)
    cells.setflags(write=False)
    return cells


# ---------------------------------------------------------------- 1. the definition
DEF_TURNS = 600
LONG_TURNS = 1100

_soups_64x16 = {}


def soups_64x16(golhip):
    """Seeds 0..255 at 64 x 16, density 1/2 (W = 1, R = 4): the cells and, under B3/S23, the repeat
    turns after 600 and after 1100 turns and the alive counts of 1100 turns.  Computed once."""
    if not _soups_64x16:
        cells = soup_cells(golhip, 64, 16, np.arange(256))
        ref, counts, _ = np_periods(cells, LIFE, LONG_TURNS, at=(DEF_TURNS,))
        _soups_64x16.update(cells=cells, ref=ref, counts=counts)
    return _soups_64x16


def test_definition(golhip):
    s = soups_64x16(golhip)
    want = records(s["ref"][DEF_TURNS], s["counts"], DEF_TURNS)
    repeated = int((want["repeat_turn"] > 0).sum())
    # the reference alone: both classes hold at least a tenth of the soups
    assert repeated >= 26 and 256 - repeated >= 26, repeated
    assert (want["stop_turn"][want["repeat_turn"] > 0] < DEF_TURNS).any()  # some soups are retired early
    with golhip.Batch(64, 16, 3) as b:  # nboards has nothing to do with nsoups
        got = b.search(256, seed0=0, max_turns=DEF_TURNS)
        check(got, want, "seed0")
        check(b.search(256, seeds=np.arange(256), max_turns=DEF_TURNS), want, "seeds")


# ---------------------------------------------------------------- 2. every wave count and word width
# (width, height, soups, density_q32, max_turns): (W, R) = (1, 1), (1, 2), (2, 4), (4, 4), (8, 4), (16, 4);
# widths of 4, 8 and 16 torus words; the sparse soups (0.04, 0.03: the per-cell seeding path) settle
# within the turns the numpy reference can afford at those sizes
SHAPES = [(64, 4, 64, HALF, 300), (128, 8, 64, HALF, 300), (64, 32, 32, HALF, 1100), (64, 64, 16, HALF, 1100),
          (256, 128, 16, 0x0A3D70A3, 300), (512, 256, 16, 0x07AE147A, 300)]


@pytest.mark.parametrize("w,h,n,density,max_turns", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_every_shape(golhip, w, h, n, density, max_turns):
    seeds = np.arange(n, dtype=np.uint64)
    cells = soup_cells(golhip, w, h, seeds, density)
    want = np_records(cells, LIFE, max_turns)
    # the reference alone: soups that are retired before max_turns, and soups that run to the end
    assert (want["stop_turn"] < max_turns).any() and (want["repeat_turn"] < 0).any(), want["repeat_turn"]
    with golhip.Batch(w, h, 1) as b:
        check(b.search(n, seeds=seeds, density_q32=density, max_turns=max_turns), want)


@pytest.mark.parametrize("density", [HALF, 0x028F5C28], ids=["half", "sparse"])
def test_512x512_against_the_batch_period_path(golhip, density):
    """(W, R) = (16, 8): four soups, 150 turns, against init_random + track_period + step + periods
    and the step's history.  The sparse soups (0.01) die or freeze within a few turns."""
    seeds, max_turns = np.array([5, 6, 7, 8], dtype=np.uint64), 150
    with golhip.Batch(512, 512, 4) as b:
        b.init_random(seeds=seeds, density_q32=density)
        b.track_period()
        counts = b.step(max_turns, history=True)
        repeat_turn, period = b.periods()
        want = records(repeat_turn, counts, max_turns)
        assert np.array_equal(want["period"], period)
        assert (repeat_turn > 0).all() if density != HALF else (repeat_turn < 0).all(), repeat_turn
        before = b.store()
        check(b.search(4, seeds=seeds, density_q32=density, max_turns=max_turns), want)
        assert np.array_equal(b.store(), before) and b.turn == max_turns


# ---------------------------------------------------------------- 3. the stop logic at every remainder
@pytest.mark.parametrize("w,h", [(64, 16), (64, 64), (512, 256)], ids=["1wave", "4waves", "16waves"])
def test_empty_boards_stop_at_every_remainder(golhip, w, h):
    """Density 0: the board is empty, the repeat (1, 1), and the soup stops at min(max_turns, f(1))."""
    assert f(1) == 40
    with golhip.Batch(w, h, 1) as b:
        for max_turns in [*range(1, 71), 95, 96, 97, 127, 128, 129, 1 << 20]:
            got = b.search(3, seed0=9, density_q32=0, max_turns=max_turns)
            for name, value in zip(FIELDS, (1, 1, min(max_turns, 40), 0, 0)):
                assert (got[name] == value).all(), (max_turns, name, got[name])


def test_a_repeat_in_the_last_turns(golhip):
    """Eight soups of test 1 with repeat turn r: max_turns = r - 1 ends without a repeat, r and r + 1
    find it -- in the last, partial block of generations, at every position the block can end."""
    s = soups_64x16(golhip)
    repeat, counts = s["ref"][LONG_TURNS], s["counts"]
    assert np.array_equal(s["ref"][DEF_TURNS], np.where(repeat <= DEF_TURNS, repeat, -1))
    picked = []
    for r in (512, 513, 1025, 128, 129, 256, 257, 133):  # block ends and block starts first
        hit = np.nonzero(repeat == r)[0]
        if hit.size:
            picked.append(int(hit[0]))
    for i in np.nonzero(repeat > 0)[0]:  # then any other repeat turn not yet taken
        if len(picked) < 8 and repeat[i] not in repeat[picked] and repeat[i] < LONG_TURNS:
            picked.append(int(i))
    assert len(picked) == 8, repeat
    # the reference alone: a repeat on a block's last generation and one on a block's first
    assert (repeat[picked] % 32 == 0).any() and (repeat[picked] % 32 == 1).any(), repeat[picked]
    with golhip.Batch(64, 16, 1) as b:
        for i in picked:
            r = int(repeat[i])
            p = int(period_of([r])[0])
            for max_turns, want in ((r - 1, (-1, -1, r - 1)), (r, (r, p, r)), (r + 1, (r, p, r + 1))):
                got = b.search(1, seeds=[i], max_turns=max_turns)[0]
                want = (*want, int(counts[i, max_turns - 1]), 0)
                assert tuple(int(got[name]) for name in FIELDS) == want, (i, r, max_turns, got)


# ---------------------------------------------------------------- 4. rules
def test_highlife_is_the_folded_form(golhip):
    s = soups_64x16(golhip)
    want = np_records(s["cells"], HIGHLIFE, DEF_TURNS)
    assert (want["repeat_turn"] > 0).any() and (want["repeat_turn"] < 0).any()
    with golhip.Batch(64, 16, 2, rule="B36/S23") as b:
        assert b.kernel_form == 1
        check(b.search(256, max_turns=DEF_TURNS), want)


def test_the_table_form(golhip):
    """B38/S0236: lone cells survive and dense soups burn on -- no soup repeats."""
    s = soups_64x16(golhip)
    want = np_records(s["cells"][:64], TABLE_RULE, 300)
    assert (want["repeat_turn"] < 0).all()
    with golhip.Batch(64, 16, 2, rule=TABLE_RULE) as b:
        assert b.kernel_form == 2
        check(b.search(64, max_turns=300), want)


def test_a_b0_rule_strobes(golhip):
    """B03/S23 on an empty board: full, empty, full, ...: the repeat is (3, 2)."""
    with golhip.Batch(64, 16, 1, rule=STROBE) as b:
        for max_turns, want in ((2, (-1, -1, 2, 0, 0)), (3, (3, 2, 3, 64 * 16, 0)), (41, (3, 2, 40, 0, 0))):
            got = b.search(2, density_q32=0, max_turns=max_turns)
            for name, value in zip(FIELDS, want):
                assert (got[name] == value).all(), (max_turns, name, got[name])


def test_one_rule_per_soup(golhip):
    """One seed under 64 rules (B3/S23, HighLife, the table rule, the strobing rule and 60 drawn masks)
    against numpy, and equal to the records of each rule as the batch's uniform rule."""
    rng = np.random.default_rng(64)
    rules = [LIFE, HIGHLIFE, TABLE_RULE, STROBE] + [tuple(int(v) for v in rng.integers(0, 512, 2)) for _ in range(60)]
    seed, max_turns = 17, 300
    cells = np.repeat(soup_cells(golhip, 64, 16, [seed]), 64, axis=0)
    want = np_records(cells, rules, max_turns)
    assert len(set(want["repeat_turn"])) >= 4, want["repeat_turn"]
    with golhip.Batch(64, 16, 64, rules=[STROBE] * 64) as b:  # the handle's per-board rules are not the soups'
        got = b.search(64, seeds=[seed] * 64, max_turns=max_turns, rules=rules)
        check(got, want)
        texts = [golhip.rule_string(*r) for r in rules]
        assert np.array_equal(b.search(64, seeds=[seed] * 64, max_turns=max_turns, rules=texts), got)
        assert b.kernel_form == 3 and np.array_equal(b.rules, [STROBE] * 64)
        b.set_rules(None)
        for i, rule in enumerate(rules):
            b.set_rule(rule)
            one = b.search(1, seeds=[seed], max_turns=max_turns)
            assert one[0] == got[i], (i, rule, one[0], got[i])


# ---------------------------------------------------------------- 5. independence
def test_records_do_not_depend_on_position(golhip):
    s = soups_64x16(golhip)
    want = records(s["ref"][DEF_TURNS], s["counts"], DEF_TURNS)
    perm = np.random.default_rng(5).permutation(256)
    with golhip.Batch(64, 16, 1) as b:
        got = b.search(256, seeds=perm, max_turns=DEF_TURNS)
    check(got, {name: v[perm] for name, v in want.items()})


def test_records_do_not_depend_on_the_chunks(golhip):
    """65536 + 37 soups of 64 x 4 cross a chunk boundary: the first and the last 512 records are those
    of 512-soup searches of the same seeds."""
    n, seed0, max_turns = 65536 + 37, 1 << 40, 64
    with golhip.Batch(64, 4, 2) as b:
        got = b.search(n, seed0=seed0, max_turns=max_turns)
        first = b.search(512, seed0=seed0, max_turns=max_turns)
        last = b.search(512, seeds=np.uint64(seed0) + np.arange(n - 512, n, dtype=np.uint64), max_turns=max_turns)
    assert got.shape == (n,)
    assert np.array_equal(got[:512], first) and np.array_equal(got[-512:], last)
    cells = soup_cells(golhip, 64, 4, np.uint64(seed0) + np.arange(n - 64, n, dtype=np.uint64))
    want = np_records(cells, LIFE, max_turns)
    assert (want["repeat_turn"] > 0).any()
    check(got[-64:], want)
    assert (got["stop_turn"] == stop_turn_of(got["repeat_turn"], max_turns)).all()
    assert (got["period"] == period_of(got["repeat_turn"])).all() and (got["reserved"] == 0).all()


# ---------------------------------------------------------------- 6. the handle is untouched
def test_search_leaves_the_handle_as_it_was(golhip):
    cells = soups(5, 64, 64, 23)
    runs = []
    for searched in (False, True):
        with golhip.Batch(64, 64, 5, rule=HIGHLIFE) as b:
            b.load(cells * 255)
            b.track_period()
            b.step(37)
            state = (b.store(), b.turn, b.periods(), b.rule_masks, b.kernel_form)
            if searched:
                got = b.search(100, seed0=3, max_turns=200)
                assert got.shape == (100,)
                after = (b.store(), b.turn, b.periods(), b.rule_masks, b.kernel_form)
                assert np.array_equal(after[0], state[0]) and after[1] == state[1] == 37
                assert np.array_equal(after[2][0], state[2][0]) and np.array_equal(after[2][1], state[2][1])
                assert after[3:] == state[3:] == (HIGHLIFE, 1)
            b.step(100)
            runs.append((b.store(), b.turn, *b.periods()))
    assert runs[0][1] == runs[1][1] == 137
    for a, c in zip(runs[0], runs[1]):
        assert np.array_equal(a, c)
    ref, _, end = np_periods(cells, HIGHLIFE, 137)
    assert np.array_equal(runs[1][2], ref[137]) and np.array_equal((runs[1][0] != 0).astype(np.uint8), end)


# ---------------------------------------------------------------- 7. errors
def test_errors(golhip):
    lib = golhip.load_library()
    with golhip.Batch(16, 16, 2) as b:  # init_random's condition
        with pytest.raises(golhip.GolHipError) as ei:
            b.search(4, max_turns=10)
        assert ei.value.code == golhip.ERR_ARG and "width" in str(ei.value)
    cells = soups(2, 64, 16, 3)
    with golhip.Batch(64, 16, 2) as b:
        b.load(cells * 255)
        b.step(5)
        state = (b.store(), b.turn)
        out = np.full(4, 7, dtype=golhip.SOUP_DTYPE)
        untouched = out.copy()
        good = np.array([8, 8, 8, 8], dtype=np.uint32)
        bad = np.array([8, 8, 0x208, 8], dtype=np.uint32)

        def call(nsoups=4, max_turns=10, birth=None, survive=None, out=out):
            return lib.golhip_batch_search(b._h, nsoups, None, 0, HALF, max_turns,
                                           None if birth is None else birth.ctypes.data,
                                           None if survive is None else survive.ctypes.data,
                                           None if out is None else out.ctypes.data)

        for kwargs, words in ((dict(max_turns=0), ["max_turns"]), (dict(max_turns=(1 << 20) + 1), ["max_turns"]),
                              (dict(max_turns=-3), ["max_turns"]), (dict(nsoups=-1), ["nsoups"]),
                              (dict(birth=bad, survive=good), ["soup 2", "0x208"]),
                              (dict(birth=good, survive=bad), ["soup 2", "0x208"]),
                              (dict(birth=good), ["birth", "survive"]), (dict(survive=good), ["birth", "survive"]),
                              (dict(out=None), ["out"])):
            assert call(**kwargs) == golhip.ERR_ARG, kwargs
            why = lib.golhip_batch_last_error(b._h).decode()
            assert all(word in why for word in words), (kwargs, why)
            assert np.array_equal(out, untouched), kwargs
            assert np.array_equal(b.store(), state[0]) and b.turn == state[1], kwargs
        for kwargs in (dict(max_turns=0), dict(max_turns=(1 << 20) + 1), dict(nsoups=-1),
                       dict(rules=[LIFE, (0x208, 8), LIFE, LIFE]), dict(rules=[LIFE] * 3), dict(seeds=[1, 2, 3])):
            with pytest.raises(golhip.GolHipError) as ei:
                b.search(**{"nsoups": 4, "max_turns": 10, **kwargs})
            assert ei.value.code == golhip.ERR_ARG, kwargs
        # no soups: a no-op, whatever out is
        assert call(nsoups=0, out=None) == golhip.OK and call(nsoups=0) == golhip.OK
        assert np.array_equal(out, untouched)
        assert b.search(0, max_turns=10).shape == (0,)
        # the handle still works
        assert call() == golhip.OK and not np.array_equal(out, untouched)
        assert np.array_equal(out, b.search(4, max_turns=10))
        want = np_records(soup_cells(golhip, 64, 16, np.arange(4)), LIFE, 10)
        check(out, want)
        assert np.array_equal(b.store(), state[0]) and b.turn == state[1]
        b.step(3)
        assert b.turn == 8
