"""The exact soup search without a GPU: golhip_batch_search_exact is exported, declared and bound,
the ABI version moved, golhip.Batch has the interface, cycle_start_floor is the documented bound,
the new kernel translation units are built and guarded against scratch, and the production library
still passes the boundary checks with them in it."""
import re
import subprocess

import test_boundary
from conftest import PKG, ROOT

FUNCTION = "golhip_batch_search_exact"


def test_library_exports_the_function(golhip):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / "lib" / "libgolhip.so")], text=True)
    exported = set(re.findall(r" T (golhip_\w+)", out))
    header = (ROOT / "include" / "golhip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*(golhip_\w+)\s*\(", header, re.M))
    assert FUNCTION in exported and FUNCTION in declared and FUNCTION in golhip.EXPORTS
    assert declared == set(golhip.EXPORTS)
    lib = golhip.load_library()
    assert len(lib.golhip_batch_search_exact.argtypes) == 10
    assert len(lib.golhip_batch_search.argtypes) == 9  # the plain search is what it was
    assert lib.golhip_version() >= 110  # 109: topology and the soup box


def test_the_header_states_the_contract():
    header = " ".join((ROOT / "include" / "golhip.h").read_text().replace(" *", " ").split())
    for phrase in ("0 <= cycle_start <= repeat_turn - period",
                   "cycle_start + period <= repeat_turn <= max_turns",
                   "cycle_start == 0 exactly when",
                   "cycle_start == NULL with nsoups > 0 is GOLHIP_ERR_ARG",
                   "out is byte for byte what golhip_batch_search writes",
                   "first golhip_batch_search or golhip_batch_search_exact",
                   "a HighLife search runs its exact pass in the table form"):
        assert phrase in header, phrase


def test_batch_has_the_interface(golhip):
    assert callable(golhip.Batch.search_exact) and callable(golhip.Batch.search)
    doc = golhip.Batch.search_exact.__doc__
    for word in ("cycle_start", "records", "repeat_turn", "period", "-1", "cycle_start_floor"):
        assert word in doc, word


def test_the_documented_floor(golhip):
    f = golhip.cycle_start_floor
    assert f(1, 1) == 0
    assert f(3, 2) == 0
    assert f(2048, 1) == 1023
    assert f(2049, 2) == 1023
    assert f(1023 + 600, 600) == 0
    assert f(-1, -1) == 0
    # every record Brent's scheme can produce: repeat_turn = 2^j - 1 + period, period <= 2^j
    for j in range(0, 12):
        s = (1 << j) - 1
        for p in sorted({1, 2, 3, (1 << j) // 2, (1 << j) // 2 + 1, 1 << j} - {0}):
            if p > 1 << j:
                continue
            lo = f(s + p, p)
            assert 0 <= lo <= s, (j, p, lo)
            if j > 0 and p <= 1 << (j - 1):
                assert lo == (1 << (j - 1)) - 1, (j, p, lo)  # the previous snapshot turn
            else:
                assert lo == 0, (j, p, lo)
    # and any pair of integers at all stays inside the bounds
    for r in range(1, 200):
        for p in range(1, r + 1):
            assert 0 <= f(r, p) <= r - p, (r, p)


def test_batch_cycle_sources_are_in_the_build_and_the_scratch_guard():
    make = (PKG / "Makefile").read_text()
    assert (PKG / "csrc" / "batch_cycle.hpp").exists()
    sources = sorted(p.name for p in (PKG / "csrc").glob("batch_cycle*.hip"))
    assert sources == ["batch_cycle.hip"]  # both functors in one translation unit: the library's size
    text = (PKG / "csrc" / "batch_cycle.hip").read_text()
    assert "launch_batch_cycle_as<LifeNext>" in text and "launch_batch_cycle_as<RuleTable>" in text
    guard = [line for line in make.splitlines() if "--scratch-only" in line and "$(OUT)/stencil_board.o" in line]
    assert guard and all("$(BATCH_CYCLE_OBJS)" in line for line in guard)
    for kept in ("$(BATCH_RULE_OBJS)", "$(BATCH_PERIOD_OBJS)", "$(BATCH_SEARCH_OBJS)", "$(BATCH_PLANE_OBJS)",
                 "$(RULE_OBJS)"):
        assert all(kept in line for line in guard), kept
    expanded = subprocess.check_output(["make", "-s", "-n", "-B", "-C", str(PKG), "guard"], text=True)
    guard_cmds = [line for line in expanded.splitlines() if "--scratch-only" in line and "stencil_board.o" in line]
    assert guard_cmds
    for src in sources:
        obj = "lib/" + src.replace(".hip", ".o")
        assert "csrc/" + src in expanded, src           # compiled
        assert all(obj in line for line in guard_cmds), src  # and guarded
    log = (PKG / "lib" / "vmcnt_guard.log")
    assert log.exists() and "0 use scratch" in log.read_text().splitlines()[-1]


def test_the_exact_pass_leaves_the_other_kernel_sources_alone():
    """The pass includes the search's headers; it does not sit in their translation units."""
    csrc = PKG / "csrc"
    for pattern in ("batch_search_*.hip", "batch_plane_*.hip", "batch_period_*.hip", "batch_rule_*.hip"):
        for p in csrc.glob(pattern):
            assert "gol_batch_cycle" not in p.read_text(), p.name
    assert "gol_batch_cycle" in (csrc / "batch_cycle.hpp").read_text()


def test_production_sources_still_pass_the_boundary_checks(golhip):
    """The same checks as tests/test_boundary.py, run here because this change adds production
    sources (batch_cycle.hpp, batch_cycle_*.hip) and an export: the production library with the 16
    new kernels is still less than a third of the tuning library."""
    test_boundary.test_production_sources_never_name_the_tuning_build()
    test_boundary.test_production_library_reads_only_documented_hooks()
    test_boundary.test_library_exports_every_declared_symbol(golhip)
    test_boundary.test_tuning_library_exports_the_same_abi(golhip)
