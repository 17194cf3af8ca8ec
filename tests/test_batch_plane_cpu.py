"""Plane topology and the soup box without a GPU: the four functions are exported, declared, bound
and in EXPORTS, the ABI version moved, golhip.Batch has the interface and its docstrings name it,
the new kernel translation units are built and guarded against scratch, and the production library
still passes the boundary checks with them in it."""
import re
import subprocess

import test_boundary
from conftest import PKG, ROOT

FUNCTIONS = ("golhip_batch_set_topology", "golhip_batch_get_topology", "golhip_batch_set_soup_box",
             "golhip_batch_get_soup_box")


def test_library_exports_the_functions(golhip):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / "lib" / "libgolhip.so")], text=True)
    exported = set(re.findall(r" T (golhip_\w+)", out))
    header = (ROOT / "include" / "golhip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*(golhip_\w+)\s*\(", header, re.M))
    lib = golhip.load_library()
    for name in FUNCTIONS:
        assert name in exported and name in declared and name in golhip.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert declared == set(golhip.EXPORTS)
    assert len(lib.golhip_batch_set_topology.argtypes) == 2 and len(lib.golhip_batch_set_soup_box.argtypes) == 3
    assert lib.golhip_version() >= 109  # 108: the soup search
    assert re.search(r"#define GOLHIP_TOPOLOGY_TORUS 0\b", header) and re.search(r"#define GOLHIP_TOPOLOGY_PLANE 1\b", header)
    assert (golhip.TOPOLOGY_TORUS, golhip.TOPOLOGY_PLANE) == (0, 1)


def test_the_header_states_the_contract():
    header = " ".join((ROOT / "include" / "golhip.h").read_text().replace(" *", " ").split())
    for phrase in ("HighLife on a plane runs the table form", "the topology and the soup box",
                   "x0 = (width - box_w) / 2", "golhip_batch_load_bytes ignores it"):
        assert phrase in header, phrase


def test_batch_has_the_interface(golhip):
    assert callable(golhip.Batch.set_topology) and callable(golhip.Batch.set_soup_box)
    assert isinstance(golhip.Batch.topology, property) and isinstance(golhip.Batch.soup_box, property)
    for doc, words in ((golhip.Batch.__doc__, ("topology", "soup_box", "set_topology", "set_soup_box", "plane")),
                       (golhip.Batch.search.__doc__, ("topology", "soup_box", "plane")),
                       (golhip.Batch.set_topology.__doc__, ("torus", "plane", "turn 0")),
                       (golhip.Batch.set_soup_box.__doc__, ("init_random", "search", "load")),
                       (golhip.Batch.init_random.__doc__, ("soup_box",))):
        for word in words:
            assert word in doc, word


def test_a_bad_topology_name_fails_before_a_handle_exists(golhip):
    try:
        golhip.Batch(64, 64, 1, topology="klein")
    except golhip.GolHipError as e:  # raised before golhip_batch_create: no device is touched
        assert e.code == golhip.ERR_ARG and "klein" in str(e)
    else:
        raise AssertionError("topology 'klein' was accepted")


def test_batch_plane_sources_are_in_the_build_and_the_scratch_guard():
    make = (PKG / "Makefile").read_text()
    assert (PKG / "csrc" / "batch_plane.hpp").exists()
    sources = sorted(p.name for p in (PKG / "csrc").glob("batch_plane_*.hip"))
    # B3/S23's rule step, the table form, the soup box's clip pass
    assert sources == [f"batch_plane_{f}.hip" for f in ("box", "life", "table")]
    guard = [line for line in make.splitlines() if "--scratch-only" in line and "$(OUT)/stencil_board.o" in line]
    assert guard and all("$(BATCH_PLANE_OBJS)" in line for line in guard)
    for kept in ("$(BATCH_RULE_OBJS)", "$(BATCH_PERIOD_OBJS)", "$(BATCH_SEARCH_OBJS)", "$(RULE_OBJS)"):
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


def test_production_sources_still_pass_the_boundary_checks(golhip):
    """The same checks as tests/test_boundary.py, run here because this change adds production
    sources (batch_plane.hpp, batch_plane_*.hip) and four exports."""
    test_boundary.test_production_sources_never_name_the_tuning_build()
    test_boundary.test_production_library_reads_only_documented_hooks()
    test_boundary.test_library_exports_every_declared_symbol(golhip)
    test_boundary.test_tuning_library_exports_the_same_abi(golhip)
