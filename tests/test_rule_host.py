"""CPU tests of life-like rules on the batch (include/gol/gol.h gol_rule_parse, gol_rule_format, gol_ensemble_set_rule,
gol_ensemble_rule): the parser, the formatter and the bit-sliced evaluator under the sanitizers, the names in every
binding, and the numpy reference of tests/test_gpu_rules.py against the CPU oracle.  No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gameoflifewithactors_amd", "csrc")
NAMES = ("gol_rule_parse", "gol_rule_format", "gol_ensemble_set_rule", "gol_ensemble_rule")


def test_rules_under_sanitizers(tmp_path):
    """tests/cpp/test_rule.cpp (its own main) with the address and undefined-behaviour sanitizers: format then parse
    is the identity on all 2^18 rules, every malformed text is refused with the outputs untouched, and the bit-sliced
    evaluator equals the scalar definition on all 2^9 neighbourhoods under all 2^18 rules (and life_next under
    B3/S23)."""
    exe = tmp_path / "test_rule"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "test_rule.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rule evaluator: 4194304 words" in r.stdout  # 2^18 rules x 16 words of 32 neighbourhoods
    assert "rules ok: 262144 rules, 512 neighbourhoods" in r.stdout


def test_the_rule_header_has_no_hip():
    """gol_rule.h is host code a plain g++ compiles (the sanitizer program above does): nothing of HIP in it."""
    src = open(os.path.join(CSRC, "gol_rule.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("#include <hip", "__builtin_amdgcn", "threadIdx", "__device__", "__global__", "__host__", "hipError"):
        assert word not in code, word
    assert "#include" not in code.replace("#include <stdint.h>", "")  # and it stands alone
    for user in ("gol_batch.cpp", "gol_batch.hip", "gol_cycles.hip"):
        assert '#include "gol_rule.h"' in open(os.path.join(CSRC, user)).read(), user


def test_rules_are_named_in_every_binding():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "gol", "gol.h")).read()
    assert re.search(r"(?m)^int\s+gol_rule_parse\s*\(const char\*\s*text,\s*int\*\s*birth,\s*int\*\s*survive\);", header)
    assert re.search(r"(?m)^int\s+gol_rule_format\s*\(int birth,\s*int survive,\s*char\*\s*out,\s*int64_t len\);", header)
    assert re.search(r"(?m)^int\s+gol_ensemble_set_rule\s*\(gol_batch\*\s*b,\s*int birth,\s*int survive\);", header)
    assert re.search(r"(?m)^int\s+gol_ensemble_rule\s*\(gol_batch\*\s*b,\s*int\*\s*birth,\s*int\*\s*survive\);", header)
    assert re.search(r"(?m)^#define\s+GOL_RULE_LIFE_BIRTH\s+0x008\b", header)
    assert re.search(r"(?m)^#define\s+GOL_RULE_LIFE_SURVIVE\s+0x00C\b", header)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fsharp = open(os.path.join(ROOT, "bindings", "fsharp", "GolNative.fs")).read()
    host = open(os.path.join(ROOT, "include", "gol", "gol_host.hpp")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int, name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, fsharp), name
        assert name in host and name in doc, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 4, 3, 3]
    assert hasattr(lib, "gol_debug_batch_rule_table") and "gol_debug_batch_rule_table" in _lib.SIGNATURES
    assert "gol_debug_batch_rule_table" in open(os.path.join(CSRC, "gol_debug.h")).read()
    assert "gol_debug_batch_rule_table" not in header  # a test knob: not part of the boundary
    assert callable(g.BoardBatch.set_rule) and isinstance(g.BoardBatch.rule, property)
    assert "batch's rule" in g.BoardBatch.cycles.__doc__ and "B3/S23 generation" not in g.BoardBatch.cycles.__doc__
    assert "under the batch's rule" in header and "next B3/S23 generation" not in header
    assert any(h.endswith("gol_rule.h") for h in build.HEADERS)


def test_batch_rule_calls_refuse_a_null_batch_without_a_device():
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    assert lib.gol_ensemble_set_rule(None, 8, 12) == _lib.GOL_ERR_INVALID
    assert b"null batch" in lib.gol_last_error()
    b, s = ctypes.c_int(77), ctypes.c_int(78)
    assert lib.gol_ensemble_rule(None, ctypes.byref(b), ctypes.byref(s)) == _lib.GOL_ERR_INVALID
    assert b"null batch" in lib.gol_last_error()
    assert (b.value, s.value) == (77, 78)
    assert lib.gol_debug_batch_rule_table(None, 1) == _lib.GOL_ERR_INVALID


def test_parse_and_format_through_ctypes():
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    assert _lib.rule_parse("B3/S23") == (0x008, 0x00C) == _lib.rule_parse(" s23/b3 ") == _lib.rule_parse("23/3")
    assert _lib.rule_parse("B36/S23") == (0x048, 0x00C)
    assert _lib.rule_parse("B3678/S34678") == (0x1C8, 0x1D8)
    assert _lib.rule_parse("B2/S") == (4, 0) and _lib.rule_parse("B/S") == (0, 0) == _lib.rule_parse("/")
    assert _lib.rule_parse(b"B0/S8") == (1, 256)
    assert _lib.rule_format(0x008, 0x00C) == "B3/S23" and _lib.rule_format(0x048, 12) == "B36/S23"
    assert _lib.rule_format(0, 0) == "B/S" and _lib.rule_format(0x1FF, 0x1FF) == "B012345678/S012345678"
    rng = np.random.default_rng(1)
    for birth, survive in rng.integers(0, 512, (200, 2)):
        assert _lib.rule_parse(_lib.rule_format(int(birth), int(survive))) == (birth, survive)
    for text in ("", "B9/S23", "B33/S23", "B3S23", "B3/S23/3", "B3/S23x", "Conway", "B3/S23" + " " * 26):
        b, s = ctypes.c_int(-5), ctypes.c_int(-6)
        assert lib.gol_rule_parse(text.encode(), ctypes.byref(b), ctypes.byref(s)) == _lib.GOL_ERR_INVALID, text
        assert lib.gol_last_error().startswith(b"rule: ") and (b.value, s.value) == (-5, -6), text
        with pytest.raises(ValueError, match="rule"):
            _lib.rule_parse(text)
    b, s = ctypes.c_int(-5), ctypes.c_int(-6)
    assert lib.gol_rule_parse(None, ctypes.byref(b), ctypes.byref(s)) == _lib.GOL_ERR_INVALID
    assert lib.gol_rule_parse(b"B3/S23", None, ctypes.byref(s)) == _lib.GOL_ERR_INVALID and s.value == -6
    buf = ctypes.create_string_buffer(b"?" * 40, 41)
    for args in ((0x200, 0, buf, 22), (0, -1, buf, 22), (8, 12, buf, 21), (8, 12, None, 22), (8, 12, buf, -1)):
        assert lib.gol_rule_format(*args) == _lib.GOL_ERR_INVALID, args[:2]
        assert buf.raw[:40] == b"?" * 40
    with pytest.raises(ValueError):
        _lib.rule_format(512, 0)
    assert lib.gol_rule_format(0x1FF, 0x1FF, buf, 22) == 0
    assert buf.raw[:23] == b"B012345678/S012345678\0?"  # 22 bytes written, not one more


@pytest.mark.parametrize("boundary", [0, 1])
def test_the_numpy_reference_is_the_oracle_under_b3s23(oracle, boundary):
    """tests/test_gpu_rules.py checks the GPU against its own numpy step; under B3/S23 that step is the CPU oracle's,
    so the new reference hangs on the one everything else is checked against."""
    import test_gpu_rules as ref

    assert ref.masks("B3/S23") == (0x008, 0x00C) and ref.masks("B3678/S34678") == (0x1C8, 0x1D8)
    assert ref.masks("B/S") == (0, 0) and ref.masks((5, 6)) == (5, 6)
    for w, h, seed in ((3, 3, 1), (33, 12, 2), (40, 12, 3), (100, 100, 4)):
        soups = ref._rand(3, h, w, seed)
        got = ref.ref_step(soups, "B3/S23", boundary, 7)
        for i in range(3):
            assert np.array_equal(got[i], oracle.c_run(soups[i], 7, boundary)), (w, h, i)
    # and its census is the oracle's: the pinned Conway glider of test_gpu_cycles.py
    glider = ref._board(33, 12, ref.GLIDER)
    assert ref.ref_census(glider, "B3/S23", boundary, 600) == [(0, 528, 5) if boundary == 0 else (27, 1, 4)]
