"""The batch handle without a GPU: its symbols are exported, declared and bound, the binding exposes
golhip.Batch, a bad size is refused before any device is touched, and the production sources and
library still pass the boundary checks with the new translation units in them."""
import re
import subprocess

import pytest

import test_boundary
from conftest import PKG, ROOT

BATCH_FUNCTIONS = ["golhip_batch_create", "golhip_batch_destroy", "golhip_batch_last_error",
                   "golhip_batch_load_bytes", "golhip_batch_store_bytes", "golhip_batch_init_random",
                   "golhip_batch_step", "golhip_batch_alive_counts", "golhip_batch_track_settle",
                   "golhip_batch_settled", "golhip_batch_turn"]


def test_library_exports_the_batch_functions(golhip):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / "lib" / "libgolhip.so")], text=True)
    exported = set(re.findall(r" T (golhip_\w+)", out))
    assert not [f for f in BATCH_FUNCTIONS if f not in exported]
    header = (ROOT / "include" / "golhip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*(golhip_\w+)\s*\(", header, re.M))
    assert set(BATCH_FUNCTIONS) <= declared
    assert declared == set(golhip.EXPORTS)
    assert "typedef struct golhip_batch *golhip_batch_t;" in header
    lib = golhip.load_library()
    for f in BATCH_FUNCTIONS:
        assert getattr(lib, f).argtypes is not None, f
    assert lib.golhip_version() >= 105
    for name in ("load", "init_random", "store", "step", "alive_counts", "track_settle", "settled", "turn",
                 "close", "__enter__", "__exit__"):
        assert hasattr(golhip.Batch, name), name


@pytest.mark.parametrize("args,value", [((48, 48, 4), "48"), ((64, 100, 4), "100"), ((64, 64, 0), "0"),
                                        ((64, 64, -3), "-3"), ((0, 64, 1), "width 0"), ((1024, 64, 1), "1024")])
def test_a_bad_size_is_refused_before_any_device_work(golhip, args, value):
    """Sizes outside the whole-board kernel's table and nboards < 1 are invalid arguments whose
    message names the offending value; no handle comes back (so this also holds without a GPU)."""
    with pytest.raises(golhip.GolHipError) as ei:
        golhip.Batch(*args)
    assert ei.value.code == golhip.ERR_ARG
    assert value in str(ei.value), str(ei.value)


def test_batch_sources_are_in_the_build_and_the_scratch_guard():
    make = (PKG / "Makefile").read_text()
    assert "csrc/batch_board.hip" in make and "engine_batch" in make
    guard = [line for line in make.splitlines() if "--scratch-only" in line and "$(OUT)/stencil_board.o" in line]
    assert guard and all("$(OUT)/batch_board.o" in line for line in guard)
    log = (PKG / "lib" / "vmcnt_guard.log")
    assert log.exists() and "0 use scratch" in log.read_text().splitlines()[-1]


def test_production_sources_still_pass_the_boundary_checks(golhip):
    """The same checks as tests/test_boundary.py, run here because this change adds production
    sources (batch_board.hip, engine_batch.hip, board_common.hpp) and library strings."""
    test_boundary.test_production_sources_never_name_the_tuning_build()
    test_boundary.test_production_library_reads_only_documented_hooks()
    test_boundary.test_library_exports_every_declared_symbol(golhip)
    test_boundary.test_tuning_library_exports_the_same_abi(golhip)
