"""The soup search without a GPU: golhip_batch_search is exported, declared and bound, the ABI
version moved, golhip.Batch has the interface, the Python record is the C struct, the new kernel
translation units are built and guarded against scratch, and the production library still passes
the boundary checks with them in it."""
import ctypes
import re
import subprocess

import test_boundary
from conftest import PKG, ROOT

SEARCH_FUNCTION = "golhip_batch_search"


def test_library_exports_the_search_function(golhip):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / "lib" / "libgolhip.so")], text=True)
    exported = set(re.findall(r" T (golhip_\w+)", out))
    assert SEARCH_FUNCTION in exported
    header = (ROOT / "include" / "golhip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*(golhip_\w+)\s*\(", header, re.M))
    assert SEARCH_FUNCTION in declared and SEARCH_FUNCTION in golhip.EXPORTS
    assert declared == set(golhip.EXPORTS)
    lib = golhip.load_library()
    assert len(lib.golhip_batch_search.argtypes) == 9
    assert lib.golhip_version() >= 108  # 107: the batch period functions


def test_batch_has_the_search_interface(golhip):
    assert callable(golhip.Batch.search)
    doc = golhip.Batch.search.__doc__
    for word in ("repeat_turn", "stop_turn", "population", "init_random(seeds="):
        assert word in doc, word


def test_the_python_record_is_the_c_struct(golhip):
    """golhip_soup_t: three int64 and two uint32, 32 bytes, no padding."""
    header = (ROOT / "include" / "golhip.h").read_text()
    m = re.search(r"typedef struct \{([^}]*)\} golhip_soup_t;", header)
    assert m, "golhip_soup_t is not declared"
    fields = []
    for ctype, names in re.findall(r"(int64_t|uint32_t)\s+([\w\s,]+);", m.group(1)):
        fields += [(name.strip(), ctype) for name in names.split(",")]
    assert fields == [("repeat_turn", "int64_t"), ("period", "int64_t"), ("stop_turn", "int64_t"),
                      ("population", "uint32_t"), ("reserved", "uint32_t")]
    assert ctypes.sizeof(golhip.Soup) == 32 and golhip.SOUP_DTYPE.itemsize == 32
    offset = 0
    for name, ctype in fields:  # the C layout: every member naturally aligned, in order
        field = getattr(golhip.Soup, name)
        size = 8 if ctype == "int64_t" else 4
        assert (field.offset, field.size) == (offset, size), name
        assert golhip.SOUP_DTYPE.fields[name][1] == offset and golhip.SOUP_DTYPE.fields[name][0].itemsize == size
        assert golhip.SOUP_DTYPE.fields[name][0].kind == ("i" if ctype == "int64_t" else "u")
        offset += size
    assert golhip.SOUP_DTYPE.names == tuple(name for name, _ in fields)


def test_the_documented_stop_turn(golhip):
    """stop_turn is a function of (repeat_turn, max_turns): max_turns without a repeat, else
    min(max_turns, f(repeat_turn)) with repeat_turn <= f(repeat_turn) <= repeat_turn + 96."""
    assert golhip.search_stop_turn(-1, 777) == 777
    assert golhip.search_stop_turn(1, 1 << 20) == 40 and golhip.search_stop_turn(32, 1 << 20) == 40
    assert golhip.search_stop_turn(33, 1 << 20) == 72 and golhip.search_stop_turn(513, 600) == 552
    for r in range(1, 300):
        stop = golhip.search_stop_turn(r, 1 << 20)
        assert r <= stop <= r + 96 and stop % 32 == 8
        assert golhip.search_stop_turn(r, r) == r and golhip.search_stop_turn(r, stop + 5) == stop
    header = (ROOT / "include" / "golhip.h").read_text()
    assert "32 * ((repeat_turn - 1) / 32) + 40" in header


def test_batch_search_sources_are_in_the_build_and_the_scratch_guard():
    make = (PKG / "Makefile").read_text()
    assert (PKG / "csrc" / "batch_search.hpp").exists()
    sources = sorted(p.name for p in (PKG / "csrc").glob("batch_search_*.hip"))
    assert sources == [f"batch_search_{f}.hip" for f in ("daynight", "highlife", "life", "replicator", "seeds",
                                                         "table")]  # one translation unit per functor
    guard = [line for line in make.splitlines() if "--scratch-only" in line and "$(OUT)/stencil_board.o" in line]
    assert guard and all("$(BATCH_SEARCH_OBJS)" in line for line in guard)
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
    sources (batch_search.hpp, batch_search_*.hip) and an export."""
    test_boundary.test_production_sources_never_name_the_tuning_build()
    test_boundary.test_production_library_reads_only_documented_hooks()
    test_boundary.test_library_exports_every_declared_symbol(golhip)
    test_boundary.test_tuning_library_exports_the_same_abi(golhip)
