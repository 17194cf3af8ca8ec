"""Life-like rules on a batch without a GPU: the six rule functions are exported, declared and
bound, golhip.Batch has the rule interface, a bad rule or a rules list of the wrong length is
refused before any device is touched, the new kernel translation units are built and guarded
against scratch, and the production library still passes the boundary checks with them in it."""
import re
import subprocess

import pytest

import test_boundary
from conftest import PKG, ROOT

RULE_FUNCTIONS = ["golhip_batch_set_rule", "golhip_batch_set_rule_masks", "golhip_batch_get_rule",
                  "golhip_batch_set_rules", "golhip_batch_get_rules", "golhip_batch_kernel"]


def test_library_exports_the_batch_rule_functions(golhip):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(PKG / "lib" / "libgolhip.so")], text=True)
    exported = set(re.findall(r" T (golhip_\w+)", out))
    assert not [f for f in RULE_FUNCTIONS if f not in exported]
    header = (ROOT / "include" / "golhip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*(golhip_\w+)\s*\(", header, re.M))
    assert set(RULE_FUNCTIONS) <= declared
    assert set(RULE_FUNCTIONS) <= set(golhip.EXPORTS)
    assert declared == set(golhip.EXPORTS)
    lib = golhip.load_library()
    for f in RULE_FUNCTIONS:
        assert getattr(lib, f).argtypes is not None, f
    assert lib.golhip_version() >= 106


def test_batch_has_the_rule_interface(golhip):
    for name in ("set_rule", "set_rules"):
        assert callable(getattr(golhip.Batch, name)), name
    for name in ("rule", "rule_masks", "rules", "kernel_form"):
        assert isinstance(getattr(golhip.Batch, name), property), name
    assert "Always B3/S23" not in golhip.Batch.__doc__


@pytest.mark.parametrize("kwargs,value", [(dict(rule="B9/S"), "9"), (dict(rule=(0x200, 0)), "0x200"),
                                          (dict(rule="nonsense"), "nonsense")])
def test_a_bad_rule_is_refused_before_any_device_work(golhip, kwargs, value):
    with pytest.raises(golhip.GolHipError) as ei:
        golhip.Batch(64, 64, 1, **kwargs)
    assert ei.value.code == golhip.ERR_ARG
    assert value in str(ei.value), str(ei.value)


def test_a_rules_list_of_the_wrong_length_is_refused_before_any_device_work(golhip):
    with pytest.raises(golhip.GolHipError) as ei:
        golhip.Batch(64, 64, 4, rules=["B3/S23", "B36/S23", (0x004, 0x000)])
    assert ei.value.code == golhip.ERR_ARG
    assert "3 rules" in str(ei.value) and "4 boards" in str(ei.value), str(ei.value)
    with pytest.raises(golhip.GolHipError) as ei:  # a bad rule inside the list: its index and text
        golhip.Batch(64, 64, 2, rules=["B3/S23", "B3/S29"])
    assert ei.value.code == golhip.ERR_ARG and "B3/S29" in str(ei.value) and "rules[1]" in str(ei.value)
    with pytest.raises(golhip.GolHipError) as ei:
        golhip.Batch(64, 64, 2, rules=[(8, 12), (0x400, 0)])
    assert ei.value.code == golhip.ERR_ARG and "0x400" in str(ei.value) and "rules[1]" in str(ei.value)


def test_batch_rule_sources_are_in_the_build_and_the_scratch_guard():
    make = (PKG / "Makefile").read_text()
    sources = sorted(p.name for p in (PKG / "csrc").glob("batch_rule*.hip"))
    assert len(sources) >= 2, sources  # split over translation units
    guard = [line for line in make.splitlines() if "--scratch-only" in line and "$(OUT)/stencil_board.o" in line]
    assert guard and all("$(OUT)/batch_board.o" in line for line in guard)
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
    sources (batch_rule.hpp, batch_rule_*.hip) and exports."""
    test_boundary.test_production_sources_never_name_the_tuning_build()
    test_boundary.test_production_library_reads_only_documented_hooks()
    test_boundary.test_library_exports_every_declared_symbol(golhip)
    test_boundary.test_tuning_library_exports_the_same_abi(golhip)
