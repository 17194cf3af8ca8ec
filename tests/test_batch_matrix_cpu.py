"""The case table of the batch kernel matrix (tests/batch_matrix_cases.py) without a GPU: it has a case
for every (W, R) of GOLHIP_BOARD_SHAPES and every rule of GOLHIP_RULE_CATALOGUE, parsed out of the
headers, and its inputs do what tests/test_gpu_batch_matrix.py needs them to do -- boards that have
and have not repeated at the checkpoints, histories that are checksums, soups that are retired and
soups that run on, and expected values that differ from rule to rule.  Every condition is on the
numpy references' results alone."""
import itertools
import re

import numpy as np
import pytest

import batch_matrix_cases as M
from conftest import PKG

CSRC = PKG / "csrc"
CASES = [(shape, name) for shape in M.SHAPES for name in M.RULES]
CASE_IDS = [f"{w}x{h}-{name}" for (w, h), name in CASES]


# ---------------------------------------------------------------- completeness
def macro_body(text, name):
    """The replacement text of `#define name(X) ...`, continuation lines included."""
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+" + name + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", text, re.M)
    assert m, name
    return re.sub(r"/\*.*?\*/", " ", m.group(1).replace("\\\n", " "))


def parse_pairs(text, name):
    """[(a, b)] of the X(a, b) entries of an X-macro list, and nothing else in its body."""
    body = macro_body(text, name)
    entry = r"X\(\s*(0[xX][0-9a-fA-F]+|\d+)\s*,\s*(0[xX][0-9a-fA-F]+|\d+)\s*\)"
    assert re.sub(entry, "", body).strip() == "", body  # an entry the pattern does not know is an error
    return [(int(a, 0), int(b, 0)) for a, b in re.findall(entry, body)]


def check_complete(board_shapes, catalogue):
    """The table against the two lists: a height per (W, R) and a form-1 case per catalogue rule."""
    heights = sorted(4 * w * r for w, r in board_shapes)
    assert len(set(heights)) == len(board_shapes), board_shapes
    assert sorted(h for _, h in M.SHAPES) == heights, (M.SHAPES, heights)
    form1 = sorted(M.RULES[name] for name, form in M.FORM.items() if form == 1)
    assert form1 == sorted(catalogue), (form1, catalogue)


def test_the_table_covers_every_shape_and_every_catalogue_rule():
    shapes = parse_pairs((CSRC / "board_common.hpp").read_text(), "GOLHIP_BOARD_SHAPES")
    catalogue = parse_pairs((CSRC / "golhip_internal.hpp").read_text(), "GOLHIP_RULE_CATALOGUE")
    assert len(shapes) == 8 and len(catalogue) == 4
    check_complete(shapes, catalogue)


CATALOGUE_TEXT = """
// one entry per rule
#define GOLHIP_RULE_CATALOGUE(X)                    \\
    X(0x048, 0x00C) /* HighLife     B36/S23      */ \\
    X(0x1C8, 0x1D8) /* Day & Night  B3678/S34678 */ \\
    X(0x004, 0x000) /* Seeds        B2/S         */ \\
    X(0x0AA, 0x0AA) /* Replicator   B1357/S1357  */%s
inline bool rule_catalogued(uint32_t birth, uint32_t survive) {
"""
SHAPES_TEXT = ("// by height\n"
               "#define GOLHIP_BOARD_SHAPES(X) X(16, 8) X(16, 4) X(8, 4) X(4, 4) X(2, 4) X(1, 4) X(1, 2) X(1, 1)%s\n\nx")


def test_the_completeness_check_bites():
    """The parser on strings: the lists as they are pass, a fifth catalogue rule or a ninth shape
    without a case fails, and so does a rule or a shape that went away."""
    catalogue = parse_pairs(CATALOGUE_TEXT % "", "GOLHIP_RULE_CATALOGUE")
    shapes = parse_pairs(SHAPES_TEXT % "", "GOLHIP_BOARD_SHAPES")
    assert catalogue == [(0x048, 0x00C), (0x1C8, 0x1D8), (0x004, 0x000), (0x0AA, 0x0AA)]
    assert shapes == [(16, 8), (16, 4), (8, 4), (4, 4), (2, 4), (1, 4), (1, 2), (1, 1)]
    check_complete(shapes, catalogue)
    more_rules = parse_pairs(CATALOGUE_TEXT % " \\\n    X(0x008, 0x03E) /* Maze B3/S12345 */", "GOLHIP_RULE_CATALOGUE")
    assert len(more_rules) == 5
    with pytest.raises(AssertionError):
        check_complete(shapes, more_rules)
    more_shapes = parse_pairs(SHAPES_TEXT % " X(16, 16)", "GOLHIP_BOARD_SHAPES")
    assert len(more_shapes) == 9
    with pytest.raises(AssertionError):
        check_complete(more_shapes, catalogue)
    with pytest.raises(AssertionError):
        check_complete(shapes, catalogue[:3])
    with pytest.raises(AssertionError):
        check_complete(shapes[1:], catalogue)
    with pytest.raises(AssertionError):  # an entry of another form is not skipped
        parse_pairs(SHAPES_TEXT % " X(16, 16, 2)", "GOLHIP_BOARD_SHAPES")


def test_the_rules_are_the_issue_s(golhip):
    assert M.SHAPES == [(64, 4), (128, 8), (64, 16), (256, 32), (64, 64), (512, 128), (64, 256), (64, 512)]
    texts = {name: golhip.rule_string(*rule) for name, rule in M.RULES.items()}
    assert texts == {"life": "B3/S23", "highlife": "B36/S23", "daynight": "B3678/S34678", "seeds": "B2/S",
                     "replicator": "B1357/S1357", "table": "B38/S0236"}
    assert golhip.rule_string(*M.STROBE) == "B03/S23" and len(set(M.MIX)) == 7
    assert M.FORM == {"life": 0, "highlife": 1, "daynight": 1, "seeds": 1, "replicator": 1, "table": 2}
    words = [max(4, w // 32) for w, _ in M.SHAPES]  # torus words per row
    assert [words.count(n) for n in (4, 8, 16)] == [6, 1, 1], words  # 8 and 16 words: 256 x 32 and 512 x 128
    assert [M.rotating_rule(s) for s in M.SHAPES] == ["highlife", "daynight", "seeds", "replicator", "table",
                                                      "highlife", "daynight", "seeds"]
    assert sorted({max(4, w // 32) for w, _ in M.BOXED_TORUS_SHAPES}) == [4, 8, 16]


# ---------------------------------------------------------------- the step and period boards
def longest_alive_run(counts, limit):
    best = run = 0
    for c in counts[:limit]:
        run = run + 1 if c > 0 else 0
        best = max(best, run)
    return best


@pytest.mark.parametrize("shape,name", CASES, ids=CASE_IDS)
def test_step_and_period_boards(shape, name):
    cells = M.step_boards(shape)
    want = M.torus_expected(shape, M.RULES[name])
    n, t1, t2 = cells.shape[0], want["t1"], want["t2"]
    assert 4 <= n <= 8 and t1 % 4 != 0 and t1 < t2
    assert t2 <= 200 or (name == "replicator" and shape[1] >= 128), t2
    at_t1, at_t2 = want["repeat"][t1], want["repeat"][t2]
    assert (at_t1 < 0).any(), at_t1                      # (a) a board without a repeat at t1
    assert (at_t2 > 0).any(), at_t2                      # (b) a board that has repeated at t2
    runs = [longest_alive_run(want["counts"][i], int(at_t2[i]) if at_t2[i] > 0 else t2) for i in range(n)]
    settled = want["settled"][t2]
    if name == "replicator":
        # (d) the rule forbids a board that does not settle: every board is dead at turn max(width,
        # height) / 2 (t2_of), the tiled one at 32, and settles two turns later; t2 is past that.  At
        # t1 the tiled board has settled and the others have not, except where all die at turn 32
        dead = max(shape) // 2
        assert (settled == np.where(np.arange(n) == n - (2 if M.big(shape) else 3), 34, dead + 2)).all(), settled
        assert t2 > dead + 2 and (want["counts"][:, dead - 1:] == 0).all() and (want["counts"][0, :dead - 1] > 0).all()
        assert (want["settled"][t1] < 0).any() and ((want["settled"][t1] > 0).any() or dead == 32)
    else:
        assert (settled > 0).any() and (settled < 0).any(), settled  # (d) one settles, one does not
    if name == "replicator" and max(shape) == 64:
        # (c) the rule forbids it here: dead at turn 32, no history is alive for more than 31 turns
        assert max(runs) == 31, runs
    else:
        assert max(runs) >= 32, runs                     # (c) a history that is a checksum
    assert not np.array_equal(want["at_t1"], want["at_t2"])


# ---------------------------------------------------------------- the search calls
@pytest.mark.parametrize("shape,name", CASES, ids=CASE_IDS)
def test_search_calls(shape, name):
    calls = M.search_calls(shape, name)
    assert 1 <= len(calls) <= 2 and calls[0] == M.shared_call(shape)
    retired = runs_on = 0
    for seeds, density_q32, max_turns in calls:
        # 4 soups in Replicator's call of 530 turns at 512 x 128 and 64 x 512: numpy's time
        cut = name == "replicator" and max(shape) == 512 and max_turns > 200
        assert (4 if cut else 16) <= len(seeds) <= 32 and len(set(seeds)) == len(seeds)
        assert density_q32 > 0  # no case needs the empty soup
        # Replicator's soups repeat at turn max(width, height): the call above it is longer there
        assert max_turns <= 200 or (name == "replicator" and max(shape) >= 256), max_turns
        want = M.search_expected(shape, M.RULES[name], (seeds, density_q32, max_turns))
        retired += int((want["stop_turn"] < max_turns).sum())                           # (e)
        if max_turns >= 16:
            runs_on += int(((want["repeat_turn"] == -1) & (want["population"] > 0)).sum())  # (f)
    assert retired >= 1 and runs_on >= 1, (retired, runs_on)


# ---------------------------------------------------------------- the wrong functor cannot pass
@pytest.mark.parametrize("shape", M.SHAPES, ids=M.SHAPE_IDS)
def test_the_rules_expect_different_things(shape):
    """The six uniform rules on the shared boards (the dense board 0 alone already) and in the shared
    search call: pairwise different histories and records."""
    call = M.shared_call(shape)
    for a, b in itertools.combinations(M.RULES, 2):
        ha, hb = (M.torus_expected(shape, M.RULES[r])["counts"] for r in (a, b))
        assert not np.array_equal(ha[0, :21], hb[0, :21]), (a, b)
        ra, rb = (M.search_expected(shape, M.RULES[r], call) for r in (a, b))
        assert any(not np.array_equal(ra[f], rb[f]) for f in ("repeat_turn", "stop_turn", "population")), (a, b)
        # and so do most soups on their own: a launcher that mixes rules up per soup shows too
        differ = (ra["population"] != rb["population"]) | (ra["repeat_turn"] != rb["repeat_turn"])
        assert differ.sum() * 2 > len(call[0]), (a, b, differ)


# ---------------------------------------------------------------- form 3, the exact pass, the plane
@pytest.mark.parametrize("shape", M.SHAPES, ids=M.SHAPE_IDS)
def test_one_rule_per_board(shape):
    n = M.step_boards(shape).shape[0]
    rules = M.mix_rules(n)
    assert len(set(rules)) == min(n, 7)
    want = M.torus_expected(shape, rules)
    assert (want["repeat"][want["t2"]] > 0).any() and (want["repeat"][want["t1"]] < 0).any()
    call = M.shared_call(shape)
    soup_rules = M.mix_rules(len(call[0]))
    assert set(soup_rules) == set(M.MIX)
    mixed = M.search_expected(shape, soup_rules, call)
    for i, rule in enumerate(soup_rules):  # soup i is soup i of its own rule's uniform call, where there is one
        if rule != M.STROBE:
            uniform = M.search_expected(shape, rule, call)
            assert all(mixed[f][i] == uniform[f][i] for f in mixed), (i, rule)


@pytest.mark.parametrize("shape", M.SHAPES, ids=M.SHAPE_IDS)
def test_exact_pass_soups(shape):
    """Under Life and under the shape's rotating rule some soup of the case's calls has a cycle start."""
    for name in ("life", M.rotating_rule(shape)):
        starts = []
        for call in M.search_calls(shape, name):
            want = M.search_expected(shape, M.RULES[name], call)
            start, period = M.cycle_expected(shape, M.RULES[name], call)
            repeated = want["repeat_turn"] >= 0
            assert (start[repeated] >= 0).all() and np.array_equal(period[repeated], want["period"][repeated])
            assert (start[repeated] <= (want["repeat_turn"] - want["period"])[repeated]).all()
            starts += start[repeated].tolist()
        assert starts and (max(starts) > 0 or name == "table"), (name, starts)


@pytest.mark.parametrize("shape", M.SHAPES, ids=M.SHAPE_IDS)
def test_plane_cases(shape):
    """The plane is not the torus on these boards, and the box is smaller than the board."""
    w, h = shape
    want = M.plane_expected(shape)
    assert want["differs_from_torus"]
    bw, bh = M.plane_box(shape)
    assert 1 <= bw < w and 1 <= bh < h
    rule = M.RULES[M.rotating_rule(shape)]
    whole = M.search_expected(shape, rule, M.plane_call(shape), plane=True)
    boxed = M.search_expected(shape, rule, M.plane_call(shape), plane=True, box=(bw, bh))
    assert any(not np.array_equal(whole[f], boxed[f]) for f in whole)
    torus = M.search_expected(shape, rule, M.plane_call(shape))
    assert any(not np.array_equal(whole[f], torus[f]) for f in whole)
    if shape in M.BOXED_TORUS_SHAPES:
        boxed_torus = M.search_expected(shape, rule, M.plane_call(shape), box=(bw, bh))
        assert any(not np.array_equal(boxed_torus[f], torus[f]) for f in torus)
