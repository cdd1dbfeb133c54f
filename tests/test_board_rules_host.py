"""CPU tests of life-like rules on the single board (include/gol/gol.h gol_set_rule, gol_rule): the names in every
binding, the two debug knobs, and the numpy reference of tests/test_gpu_board_rules.py against the CPU oracle.  No
kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gameoflifewithactors_amd", "csrc")


def test_board_rule_calls_exist_and_refuse_a_null_board():
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    assert lib.gol_set_rule(None, 8, 12) == _lib.GOL_ERR_INVALID
    assert b"null board" in lib.gol_last_error()
    b, s = ctypes.c_int(77), ctypes.c_int(78)
    assert lib.gol_rule(None, ctypes.byref(b), ctypes.byref(s)) == _lib.GOL_ERR_INVALID
    assert b"null board" in lib.gol_last_error()
    assert (b.value, s.value) == (77, 78)


def test_the_rule_knobs_are_debug_options():
    from gameoflifewithactors_amd import _lib

    names = _lib.load().gol_debug_option_names().decode().split(",")
    for name in ("rule_table", "rule_seg_rows"):
        assert name in names and name in _lib.DEBUG_OPTIONS, name
    assert set(names) == set(_lib.DEBUG_OPTIONS)
    text = open(os.path.join(CSRC, "gol_debug.h")).read()
    assert '"rule_table"' in text and '"rule_seg_rows"' in text


def test_board_rules_are_named_in_every_binding():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib, build, driver
    import inspect

    header = open(os.path.join(ROOT, "include", "gol", "gol.h")).read()
    assert re.search(r"(?m)^int\s+gol_set_rule\s*\(gol_board\*\s*b,\s*int birth,\s*int survive\);", header)
    assert re.search(r"(?m)^int\s+gol_rule\s*\(gol_board\*\s*b,\s*int\*\s*birth,\s*int\*\s*survive\);", header)
    assert "snapshots" in header and "do not carry it" in header
    fsharp = open(os.path.join(ROOT, "bindings", "fsharp", "GolNative.fs")).read()
    host = open(os.path.join(ROOT, "include", "gol", "gol_host.hpp")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("gol_set_rule", "gol_rule"):
        assert _lib.SIGNATURES[name][0] is ctypes.c_int and len(_lib.SIGNATURES[name][1]) == 3, name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, fsharp), name
        assert re.search(r"\b%s\(" % name, host) and re.search(r"\b%s\(" % name, doc), name
    assert callable(g.Board.set_rule) and isinstance(g.Board.rule, property)
    assert "rule" in inspect.signature(g.Board.__init__).parameters
    assert "rule" in inspect.signature(driver.run).parameters
    assert "does not carry it" in g.Board.save.__doc__
    assert any(s.endswith("gol_rule_step.hip") for s in build.SOURCES)
    assert any(h.endswith("gol_rule_plan.h") for h in build.HEADERS)
    assert "Single boards stay B3/S23" not in open(os.path.join(ROOT, "README.md")).read()


def test_the_new_pass_is_appended_to_the_pass_enum():
    text = open(os.path.join(CSRC, "gol_board.h")).read()
    m = re.search(r"enum class Pass \{([^}]*)\}", text)
    names = [n.strip() for n in m.group(1).split(",")]
    assert names == ["None", "Wave", "Lanes", "Coop", "CoopRagged", "Ring", "StreamRagged", "Resident", "Bytes", "Stream",
                     "Multi", "RuleStream"]


@pytest.mark.parametrize("boundary", [0, 1])
def test_the_numpy_reference_is_the_oracle_under_b3s23(oracle, boundary):
    import rule_reference as ref

    assert ref.masks("B3/S23") == (0x008, 0x00C) and ref.masks("B3678/S34678") == (0x1C8, 0x1D8)
    assert ref.masks("B/S") == (0, 0) and ref.masks("B0/S8") == (1, 256) and ref.masks((5, 6)) == (5, 6)
    for w, h, seed in ((33, 12, 2), (100, 100, 4)):
        cells = ref.soup(w, h, seed)
        got = ref_cells = cells
        for g in range(20):  # generation by generation: every one of the 20 is the oracle's
            got = ref.ref_step(got, 0x008, 0x00C, boundary, 1)
            ref_cells = oracle.run(ref_cells, 1, boundary)
            assert np.array_equal(got, ref_cells), (w, h, g)
        assert np.array_equal(ref.ref_step(cells, 0x008, 0x00C, boundary, 20), oracle.run(cells, 20, boundary))
