"""Period tracking on a batch without a GPU: the two functions are exported, declared and bound,
the ABI version moved, golhip.Batch has the interface, the new kernel translation units are built
and guarded against scratch, and the production library still passes the boundary checks with them
in it."""
import re
import subprocess

import test_boundary
from conftest import PKG, ROOT

PERIOD_FUNCTIONS = ["golhip_batch_track_period", "golhip_batch_periods"]


def test_library_exports_the_period_functions(golhip):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / "lib" / "libgolhip.so")], text=True)
    exported = set(re.findall(r" T (golhip_\w+)", out))
    assert not [f for f in PERIOD_FUNCTIONS if f not in exported]
    header = (ROOT / "include" / "golhip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*(golhip_\w+)\s*\(", header, re.M))
    assert set(PERIOD_FUNCTIONS) <= declared
    assert set(PERIOD_FUNCTIONS) <= set(golhip.EXPORTS)
    assert declared == set(golhip.EXPORTS)
    lib = golhip.load_library()
    for f in PERIOD_FUNCTIONS:
        assert getattr(lib, f).argtypes is not None, f
    assert len(lib.golhip_batch_periods.argtypes) == 3
    assert lib.golhip_version() >= 107  # 106: the batch rule functions


def test_batch_has_the_period_interface(golhip):
    for name in ("track_period", "periods"):
        assert callable(getattr(golhip.Batch, name)), name
    assert "period" in golhip.Batch.periods.__doc__


def test_batch_period_sources_are_in_the_build_and_the_scratch_guard():
    make = (PKG / "Makefile").read_text()
    assert (PKG / "csrc" / "batch_period.hpp").exists()
    sources = sorted(p.name for p in (PKG / "csrc").glob("batch_period_*.hip"))
    assert len(sources) == 6, sources  # one translation unit per functor
    guard = [line for line in make.splitlines() if "--scratch-only" in line and "$(OUT)/stencil_board.o" in line]
    assert guard and all("$(BATCH_PERIOD_OBJS)" in line for line in guard)
    expanded = subprocess.check_output(["make", "-s", "-n", "-B", "-C", str(PKG), "guard"], text=True)
    guard_cmds = [line for line in expanded.splitlines() if "--scratch-only" in line and "stencil_board.o" in line]
    assert guard_cmds
    for src in sources:
        obj = "lib/" + src.replace(".hip", ".o")
        assert "csrc/" + src in expanded, src           # compiled
        assert all(obj in line for line in guard_cmds), src  # and guarded
    log = (PKG / "lib" / "vmcnt_guard.log")
    assert log.exists() and "0 use scratch" in log.read_text().splitlines()[-1]


def test_production_sources_still_pass_the_boundary_checks(golhip):
    """The same checks as tests/test_boundary.py, run here because this change adds production
    sources (batch_period.hpp, batch_period_*.hip) and exports."""
    test_boundary.test_production_sources_never_name_the_tuning_build()
    test_boundary.test_production_library_reads_only_documented_hooks()
    test_boundary.test_library_exports_every_declared_symbol(golhip)
    test_boundary.test_tuning_library_exports_the_same_abi(golhip)
