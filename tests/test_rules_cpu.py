"""Life-like rules without a GPU: the B.../S... parser, the mask round trip, the exports, and a
CPU model of the rule kernel's algebra (csrc/golhip_rule.hpp), restated here from its formulas and
checked against the rule's own table G[S9][mc] -- like tests/test_drift_model.py pins the drifting
sums.

Algebra: with o, k the full adder of the three rows' sum bits and p, q that of their carries, the
9-cell sum including the centre cell mc is S9 = o + 2 (k + p + 2 q); its bits are b0 = o, b1 = k ^ p,
b2 = (k & p) ^ q, b3 = k & p & q.  G[s][0] = birth bit s, G[s][1] = survive bit s - 1; the pairs
that cannot occur (s = 0 with a live centre, s = 9 with a dead one) are 0.
"""
import ctypes
import itertools
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

CATALOGUE = {"B36/S23": (0x048, 0x00C), "B3678/S34678": (0x1C8, 0x1D8), "B2/S": (0x004, 0x000),
             "B1357/S1357": (0x0AA, 0x0AA)}
RULE_SYMBOLS = ["golhip_parse_rule", "golhip_set_rule", "golhip_set_rule_masks", "golhip_get_rule"]


def masks_of(text):
    b, s = text.upper().split("/")
    return sum(1 << int(d) for d in b[1:]), sum(1 << int(d) for d in s[1:])


def G(birth, survive, s9, mc):
    if mc:
        return (survive >> (s9 - 1)) & 1 if 1 <= s9 <= 9 else 0
    return (birth >> s9) & 1 if s9 <= 8 else 0


# ---------------------------------------------------------------- parser
@pytest.mark.parametrize("text", ["B3/S23", "b36/s23", "B2/S", "B/S", "B012345678/S012345678"])
def test_parser_accepts(golhip, text):
    assert golhip.parse_rule(text) == masks_of(text)


def test_parser_default_rule_masks(golhip):
    assert golhip.parse_rule("B3/S23") == (0x008, 0x00C)
    for text, masks in CATALOGUE.items():
        assert golhip.parse_rule(text) == masks


@pytest.mark.parametrize("text", ["", "B9/S2", "B33/S2", "S23/B3", "B3S23", "B3/S23x", None])
def test_parser_rejects(golhip, text):
    lib = golhip.load_library()
    b, s = ctypes.c_uint32(77), ctypes.c_uint32(77)
    raw = None if text is None else text.encode()
    assert lib.golhip_parse_rule(raw, ctypes.byref(b), ctypes.byref(s)) == golhip.ERR_ARG
    assert (b.value, s.value) == (77, 77)  # outputs untouched
    msg = lib.golhip_last_error(None).decode()
    assert msg and (text is None or text in msg)  # names the offending text
    with pytest.raises(golhip.GolHipError) as e:
        golhip.parse_rule(text)
    assert e.value.code == golhip.ERR_ARG


def test_parser_rejects_null_outputs(golhip):
    lib = golhip.load_library()
    b = ctypes.c_uint32()
    assert lib.golhip_parse_rule(b"B3/S23", None, ctypes.byref(b)) == golhip.ERR_ARG
    assert lib.golhip_parse_rule(b"B3/S23", ctypes.byref(b), None) == golhip.ERR_ARG


def test_masks_round_trip(golhip):
    """masks -> canonical text -> parser -> the same masks, for every pair of a seeded sample and the
    corner cases; the canonical text has ascending digits."""
    rng = np.random.default_rng(11)
    pairs = [(0, 0), (0x1FF, 0x1FF), (0x008, 0x00C)] + [tuple(int(v) for v in rng.integers(0, 512, 2))
                                                       for _ in range(200)]
    for b, s in pairs:
        text = golhip.rule_string(b, s)
        assert re.fullmatch(r"B[0-8]*/S[0-8]*", text)
        assert golhip.parse_rule(text) == (b, s)
        assert golhip.parse_rule(text.lower()) == (b, s)
    assert golhip.rule_string(*golhip.parse_rule("b63/s32")) == "B36/S23"


def test_handle_calls_reject_null_handles(golhip):
    lib = golhip.load_library()
    b = ctypes.c_uint32()
    assert lib.golhip_set_rule(None, b"B3/S23") == golhip.ERR_ARG
    assert lib.golhip_set_rule_masks(None, 8, 12) == golhip.ERR_ARG
    assert lib.golhip_get_rule(None, ctypes.byref(b), ctypes.byref(b)) == golhip.ERR_ARG


# ---------------------------------------------------------------- exports
def test_header_and_libraries_export_the_rule_calls(golhip):
    text = (ROOT / "include" / "golhip.h").read_text()
    for name in RULE_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in golhip.EXPORTS
    for lib in ("lib", "lib_tuning", "lib_faults"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / lib / "libgolhip.so")], text=True)
        exported = set(re.findall(r" T (golhip_\w+)", out))
        assert set(RULE_SYMBOLS) <= exported, lib


def test_catalogue_in_the_sources_matches(golhip):
    """The X-macro catalogue of constant-folded rules (csrc/golhip_internal.hpp) holds the four rules
    the header documents, as the masks the parser gives their names."""
    src = (PKG / "csrc" / "golhip_internal.hpp").read_text()
    body = src[src.index("#define GOLHIP_RULE_CATALOGUE"):]
    body = body[:body.index("inline bool rule_catalogued")]
    got = {(int(b, 16), int(s, 16)) for b, s in re.findall(r"X\((0x[0-9A-Fa-f]+),\s*(0x[0-9A-Fa-f]+)\)", body)}
    assert set(CATALOGUE.values()) <= got
    assert (0x008, 0x00C) not in got  # B3/S23 is the production path, never gol_rule


# ---------------------------------------------------------------- the kernel's algebra
def bitop3(a, b, c, tt):
    """v_bitop3_b32 on 0/1 values: the truth table is indexed by (a << 2) | (b << 1) | c."""
    return (tt >> ((a << 2) | (b << 1) | c)) & 1


SELECT = 0xCA  # a ? b : c


def rule_tt(birth, survive, o, mc):
    """constexpr rule_tt<B, S>(o, mc): the truth table over (k, p, q) of the next state."""
    tt = 0
    for i in range(8):
        k, p, q = (i >> 2) & 1, (i >> 1) & 1, i & 1
        tt |= G(birth, survive, o + 2 * (k + p + 2 * q), mc) << i
    return tt


def rule_const_next(birth, survive, o, k, p, q, mc):
    a00 = bitop3(k, p, q, rule_tt(birth, survive, 0, 0))
    a01 = bitop3(k, p, q, rule_tt(birth, survive, 0, 1))
    a10 = bitop3(k, p, q, rule_tt(birth, survive, 1, 0))
    a11 = bitop3(k, p, q, rule_tt(birth, survive, 1, 1))
    even = bitop3(mc, a01, a00, SELECT)
    odd = bitop3(mc, a11, a10, SELECT)
    return bitop3(o, odd, even, SELECT)


def rule_table_next(birth, survive, o, k, p, q, mc):
    b = [(birth >> n) & 1 if n <= 8 else 0 for n in range(10)]
    s = [(survive >> (n - 1)) & 1 if n >= 1 else 0 for n in range(10)]
    e = []
    for t in range(5):
        g0 = bitop3(mc, s[2 * t], b[2 * t], SELECT)
        g1 = bitop3(mc, s[2 * t + 1], b[2 * t + 1], SELECT)
        e.append(bitop3(o, g1, g0, SELECT))
    b1 = k ^ p
    b2 = (k & p) ^ q
    b3 = k & p & q
    f01 = bitop3(b1, e[1], e[0], SELECT)
    f23 = bitop3(b1, e[3], e[2], SELECT)
    f = bitop3(b2, f23, f01, SELECT)
    return bitop3(b3, e[4], f, SELECT)


def test_sum_bits_of_the_decomposition():
    for o, k, p, q in itertools.product((0, 1), repeat=4):
        s9 = o + 2 * (k + p) + 4 * q
        assert s9 == o + 2 * (k ^ p) + 4 * ((k & p) ^ q) + 8 * (k & p & q)


def test_select_table():
    for a, b, c in itertools.product((0, 1), repeat=3):
        assert bitop3(a, b, c, SELECT) == (b if a else c)


def model_rules():
    rng = np.random.default_rng(5)
    return list(CATALOGUE.values()) + [(0x008, 0x00C)] + [tuple(int(v) for v in rng.integers(0, 512, 2))
                                                          for _ in range(200)]


def test_functors_match_the_rule_table():
    """Both functors give G[S9][mc] for every (o, k, p, q, mc) -- which covers all 20 (S9, mc) pairs,
    each through every carry pattern that produces it -- for the catalogue and 200 seeded rules."""
    for birth, survive in model_rules():
        seen = set()
        for o, k, p, q, mc in itertools.product((0, 1), repeat=5):
            s9 = o + 2 * (k + p + 2 * q)
            want = G(birth, survive, s9, mc)
            assert rule_const_next(birth, survive, o, k, p, q, mc) == want, (birth, survive, s9, mc)
            assert rule_table_next(birth, survive, o, k, p, q, mc) == want, (birth, survive, s9, mc)
            seen.add((s9, mc))
        assert len(seen) == 20


def test_life_tables_reduce_to_b3s23():
    """B3/S23 through the generic tables is Conway's rule (S9 == 3, or S9 == 4 and alive)."""
    for o, k, p, q, mc in itertools.product((0, 1), repeat=5):
        s9 = o + 2 * (k + p + 2 * q)
        assert rule_const_next(0x008, 0x00C, o, k, p, q, mc) == int(s9 == 3 or (s9 == 4 and mc == 1))


def test_numpy_stepper_agrees_with_the_oracle_for_life(oracle):
    """The numpy reference of the GPU rule tests, at B3/S23, against the project's oracle."""
    rng = np.random.default_rng(2)
    board = (rng.random((37, 48)) < 0.5).astype(np.uint8)
    cur = board.copy()
    for _ in range(5):
        n = sum(np.roll(np.roll(cur.astype(np.int64), dy, 0), dx, 1)
                for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
        cur = np.where(cur == 1, (0x00C >> n) & 1, (0x008 >> n) & 1).astype(np.uint8)
    got, _ = oracle.packed_run(board * 255, 5)
    assert np.array_equal(cur * 255, got)


@pytest.mark.parametrize("w,h", [(128, 1), (128, 2), (128, 3), (48, 5), (3968, 9)])
def test_numpy_stepper_agrees_with_the_oracle_on_degenerate_heights(oracle, w, h):
    """np_step / np_run of tests/test_gpu_rules.py at B3/S23 against the oracle, every one of 10
    turns and its count, on boards of 1, 2 and 3 rows (the three neighbour rows coincide), the
    replicated 48-wide torus and the two-full-chunk width: the shapes the GPU rule tests lean on."""
    from test_gpu_rules import np_run, random_cells

    board = random_cells(w, h, w * 31 + h)
    gens, counts = np_run(board, (0x008, 0x00C), 10)
    assert 0 < counts[0] < w * h  # the first turn is not trivial
    for t in range(1, 11):
        got, got_counts = oracle.packed_run(board * 255, t)
        assert np.array_equal(gens[t] * 255, got), t
        assert np.array_equal(counts[:t], got_counts.astype(np.int64)), t
