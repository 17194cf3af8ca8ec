"""Every batch kernel the library ships, launched once against numpy: the families gol_batch_rule,
gol_batch_period, gol_batch_search, gol_batch_cycle and gol_plane_rule / _period / _search under
every rule functor (LifeNext, the four constant-folded catalogue rules, RuleTable) at every (W, R) of
GOLHIP_BOARD_SHAPES.  The cases and their expected values are the table of
tests/batch_matrix_cases.py, computed by the numpy references of the existing modules;
tests/test_batch_matrix_cpu.py shows without a GPU that the table is complete and that the rules
expect different things of the same inputs.  Every comparison is exact."""
import itertools

import numpy as np
import pytest

import batch_matrix_cases as M
from test_gpu_batch_period import cells_of, check_periods
from test_gpu_batch_search import check

pytestmark = pytest.mark.gpu

UNIFORM = [(shape, name) for shape in M.SHAPES for name in M.RULES]
UNIFORM_IDS = [f"{w}x{h}-{name}" for (w, h), name in UNIFORM]
NON_LIFE = [(shape, name) for shape, name in UNIFORM if name != "life"]
NON_LIFE_IDS = [f"{w}x{h}-{name}" for (w, h), name in NON_LIFE]
EXACT = [(shape, name) for shape in M.SHAPES for name in ("life", M.rotating_rule(shape))]
EXACT_IDS = [f"{w}x{h}-{name}" for (w, h), name in EXACT]
ROTATING = [(shape, M.rotating_rule(shape)) for shape in M.SHAPES]
ROTATING_IDS = [f"{w}x{h}-{name}" for (w, h), name in ROTATING]


def same(got, want, where):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (where, bad[:8].tolist(), got[tuple(bad[:8].T)], want[tuple(bad[:8].T)])


def same_boards(b, want, where):
    bad = np.nonzero((cells_of(b) != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, (where, bad)


def run_search(b, call, want, where, **rules):
    seeds, density_q32, max_turns = call
    got = b.search(len(seeds), seeds=np.array(seeds, dtype=np.uint64), density_q32=density_q32, max_turns=max_turns,
                   **rules)
    check(got, want, where)
    return got


# ---------------------------------------------------------------- gol_batch_rule
@pytest.mark.parametrize("shape,name", NON_LIFE, ids=NON_LIFE_IDS)
def test_torus_step_route(golhip, shape, name):
    """The four modes of gol_batch_rule (history x settle), t1 turns then t2 - t1: every history count,
    the boards at both checkpoints, alive_counts() and settled()."""
    (w, h), rule = shape, M.RULES[name]
    cells, want = M.step_boards(shape), M.torus_expected(shape, M.RULES[name])
    t1, t2 = want["t1"], want["t2"]
    for history, settle in itertools.product((True, False), (True, False)):
        where = (history, settle)
        with golhip.Batch(w, h, cells.shape[0], rule=rule) as b:
            assert b.kernel_form == M.FORM[name] and b.rule_masks == rule
            b.load(cells * 255)
            if settle:
                b.track_settle()
            for done, turns, boards in ((0, t1, want["at_t1"]), (t1, t2 - t1, want["at_t2"])):
                hist = b.step(turns, history=history)
                if history:
                    same(hist, want["counts"][:, done:done + turns], (where, done))
                same_boards(b, boards, (where, done))
                same(b.alive_counts(), want["counts"][:, done + turns - 1], (where, done, "alive"))
                if settle:
                    same(b.settled(), want["settled"][done + turns], (where, done, "settled"))
            assert b.turn == t2 and b.kernel_form == M.FORM[name]


# ---------------------------------------------------------------- gol_batch_period
def period_route(b, cells, want, where=""):
    t1, t2 = want["t1"], want["t2"]
    b.load(cells * 255)
    b.track_period()
    hist = b.step(t1, history=True)
    same(hist, want["counts"][:, :t1], (where, "history"))
    check_periods(b, want["repeat"][t1], (where, t1))
    b.step(t2 - t1)
    check_periods(b, want["repeat"][t2], (where, t2))
    same_boards(b, want["at_t2"], where)


@pytest.mark.parametrize("shape,name", UNIFORM, ids=UNIFORM_IDS)
def test_torus_period_route(golhip, shape, name):
    """track_period, t1 turns with history (the history kernel), t2 - t1 without (the plain one)."""
    (w, h), rule = shape, M.RULES[name]
    cells = M.step_boards(shape)
    with golhip.Batch(w, h, cells.shape[0], rule=rule) as b:
        assert b.kernel_form == M.FORM[name]
        period_route(b, cells, M.torus_expected(shape, rule))
        assert b.kernel_form == M.FORM[name]


# ---------------------------------------------------------------- gol_batch_search
@pytest.mark.parametrize("shape,name", UNIFORM, ids=UNIFORM_IDS)
def test_torus_search(golhip, shape, name):
    """Each call of the case under the uniform rule, and the same soups with the rule given per soup,
    which runs the table form: the same bytes."""
    (w, h), rule = shape, M.RULES[name]
    with golhip.Batch(w, h, 1, rule=rule) as b:
        assert b.kernel_form == M.FORM[name]
        for call in M.search_calls(shape, name):
            got = run_search(b, call, M.search_expected(shape, rule, call), call[1:])
            per_soup = run_search(b, call, M.search_expected(shape, rule, call), (call[1:], "per soup"),
                                  rules=[rule] * len(call[0]))
            assert per_soup.tobytes() == got.tobytes(), call[1:]
        assert b.kernel_form == M.FORM[name]


# ---------------------------------------------------------------- one rule per board / per soup
@pytest.mark.parametrize("shape", M.SHAPES, ids=M.SHAPE_IDS)
def test_one_rule_per_board_and_per_soup(golhip, shape):
    w, h = shape
    cells = M.step_boards(shape)
    rules = M.mix_rules(cells.shape[0])
    with golhip.Batch(w, h, cells.shape[0], rules=rules) as b:
        assert b.kernel_form == 3
        period_route(b, cells, M.torus_expected(shape, rules))
        call = M.shared_call(shape)
        soup_rules = M.mix_rules(len(call[0]))
        run_search(b, call, M.search_expected(shape, soup_rules, call), "per soup", rules=list(soup_rules))
        assert b.kernel_form == 3


# ---------------------------------------------------------------- gol_batch_cycle
def exact_pass(golhip, b, shape, rule, call, plane=False, box=None):
    seeds, density_q32, max_turns = call
    want = M.search_expected(shape, rule, call, plane, box)
    rec = run_search(b, call, want, ("search", call[1:]))
    got, start = b.search_exact(len(seeds), seeds=np.array(seeds, dtype=np.uint64), density_q32=density_q32,
                                max_turns=max_turns)
    assert got.dtype == golhip.SOUP_DTYPE and start.dtype == np.int64 and start.shape == (len(seeds),)
    check(got, want, ("search_exact", call[1:]))
    assert got.tobytes() == rec.tobytes(), call[1:]
    want_start, want_period = M.cycle_expected(shape, rule, call, plane, box)
    repeated = want["repeat_turn"] >= 0
    assert np.array_equal(want["period"][repeated], want_period[repeated])  # the two references agree
    same(start, np.where(repeated, want_start, -1), ("cycle_start", call[1:]))


@pytest.mark.parametrize("shape,name", EXACT, ids=EXACT_IDS)
def test_exact_pass(golhip, shape, name):
    """search_exact under Life (the LifeNext cycle kernel) and under the shape's rotating rule (every
    catalogue rule reaches the table form of the cycle kernel)."""
    (w, h), rule = shape, M.RULES[name]
    with golhip.Batch(w, h, 1, rule=rule) as b:
        assert b.kernel_form == M.FORM[name]
        for call in M.search_calls(shape, name):
            exact_pass(golhip, b, shape, rule, call)


# ---------------------------------------------------------------- the plane kernels
@pytest.mark.parametrize("shape,name", ROTATING, ids=ROTATING_IDS)
def test_plane(golhip, shape, name):
    """The table form of gol_plane_rule (history + settle), gol_plane_period and gol_plane_search,
    whole boards and a boxed soup."""
    (w, h), rule = shape, M.RULES[name]
    cells, want = M.step_boards(shape), M.plane_expected(shape)
    t1, t2 = M.PLANE_T1, M.PLANE_T2
    with golhip.Batch(w, h, cells.shape[0], rule=rule, topology="plane") as b:
        assert b.kernel_form == 2 and b.topology == "plane"
        b.load(cells * 255)
        b.track_settle()
        for done, turns in ((0, t1), (t1, t2 - t1)):
            hist = b.step(turns, history=True)
            same(hist, want["counts"][:, done:done + turns], ("step", done))
            same(b.settled(), want["settled"][done + turns], ("settled", done))
        same_boards(b, want["at_t2"], "step")
        same(b.alive_counts(), want["counts"][:, -1], "alive")
        b.track_settle(False)
        period_route(b, cells, {"t1": t1, "t2": t2, **want}, "period")
        assert b.kernel_form == 2
        call = M.plane_call(shape)
        run_search(b, call, M.search_expected(shape, rule, call, plane=True), "search")
        box = M.plane_box(shape)
        b.set_soup_box(box)
        assert b.soup_box == box
        run_search(b, call, M.search_expected(shape, rule, call, plane=True, box=box), "boxed search")


@pytest.mark.parametrize("shape", M.BOXED_TORUS_SHAPES, ids=[f"{w}x{h}" for w, h in M.BOXED_TORUS_SHAPES])
def test_boxed_torus_search(golhip, shape):
    """A soup box on a torus: gol_plane_search with the torus's seams, at rows of 4, 8 and 16 words."""
    (w, h), name = shape, M.rotating_rule(shape)
    rule, call, box = M.RULES[name], M.plane_call(shape), M.plane_box(shape)
    with golhip.Batch(w, h, 1, rule=rule, soup_box=box) as b:
        assert b.kernel_form == M.FORM[name] and b.topology == "torus" and b.soup_box == box
        run_search(b, call, M.search_expected(shape, rule, call, box=box), "boxed torus search")
