"""CPU tests of the per-board rule table of a batch (include/gol/gol.h gol_ensemble_set_rules, gol_ensemble_rules): the
table's validation and packing under the sanitizers, and the two names in every binding.  No kernel is launched here;
tests/test_gpu_batch_rules.py runs the kernels."""
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gameoflifewithactors_amd", "csrc")
NAMES = ("gol_ensemble_set_rules", "gol_ensemble_rules")


def test_rule_table_validation_under_sanitizers(tmp_path):
    """tests/cpp/test_batch_rules_host.cpp (its own main) with the address and undefined-behaviour sanitizers:
    csrc/gol_batch_host.h packs a valid table word for word, and refuses a null array, n != count and a mask outside
    0..0x1FF at the first, a middle and the last entry with not one word of the table written."""
    exe = tmp_path / "test_batch_rules_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "cpp", "test_batch_rules_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batch rules host ok" in r.stdout


def test_the_batch_host_header_has_no_hip():
    """gol_batch_host.h and what it includes stay plain C++ (the program above is compiled by g++ alone)."""
    for name in ("gol_batch_host.h", "gol_rule.h", "gol_seed_rle.h"):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
        for word in ("#include <hip", "__builtin_amdgcn", "threadIdx", "__device__", "__global__", "hipError"):
            assert word not in code, (name, word)
    host = open(os.path.join(CSRC, "gol_batch_host.h")).read()
    assert "batch_rules_pack" in host and '#include "gol_rule.h"' in host
    assert "batch_rules_pack" in open(os.path.join(CSRC, "gol_batch.cpp")).read()


def test_rule_table_calls_are_named_in_every_binding():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    header = open(os.path.join(ROOT, "include", "gol", "gol.h")).read()
    assert re.search(r"(?m)^int\s+gol_ensemble_set_rules\s*\(gol_batch\*\s*b,\s*const int\*\s*birth,"
                     r"\s*const int\*\s*survive,\s*int64_t n\);", header)
    assert re.search(r"(?m)^int\s+gol_ensemble_rules\s*\(gol_batch\*\s*b,\s*int\*\s*birth,\s*int\*\s*survive,"
                     r"\s*int64_t n\);", header)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fsharp = open(os.path.join(ROOT, "bindings", "fsharp", "GolNative.fs")).read()
    host = open(os.path.join(ROOT, "include", "gol", "gol_host.hpp")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == [_lib.vp, _lib.ip, _lib.ip, ctypes.c_int64], name
        assert re.search(r"extern\s+int\s+%s\s*\(" % name, fsharp), name
        assert re.search(r"\b%s\s*\(" % name, host), name
        assert name in doc, name
    assert "setRules" in host and "rules()" in host
    assert callable(g.BoardBatch.set_rules) and isinstance(g.BoardBatch.rules, property)
    for text in ("README.md", "DESIGN.md"):
        assert "gol_ensemble_set_rules" in open(os.path.join(ROOT, text)).read(), text
    assert "4.13" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_batch_names_still_number_17():
    """The new calls are the ensemble's (gol_ensemble_*), as the rule and the census are: gol_batch_* is unchanged."""
    header = open(os.path.join(ROOT, "include", "gol", "gol.h")).read()
    names = sorted(set(re.findall(r"(?m)^\s*int\s+(gol_batch_\w+)\s*\(", header)))
    assert len(names) == 17, names
    ensemble = sorted(set(re.findall(r"(?m)^\s*int\s+(gol_ensemble_\w+)\s*\(", header)))
    assert ensemble == ["gol_ensemble_cycles", "gol_ensemble_rule", "gol_ensemble_rules", "gol_ensemble_set_rule",
                        "gol_ensemble_set_rules"]


def test_rule_table_calls_refuse_a_null_batch_without_a_device():
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    birth, survive = (ctypes.c_int * 4)(8, 8, 8, 8), (ctypes.c_int * 4)(12, 12, 12, 12)
    assert lib.gol_ensemble_set_rules(None, birth, survive, 4) == _lib.GOL_ERR_INVALID
    assert b"null batch" in lib.gol_last_error()
    out_b, out_s = (ctypes.c_int * 4)(71, 72, 73, 74), (ctypes.c_int * 4)(75, 76, 77, 78)
    assert lib.gol_ensemble_rules(None, out_b, out_s, 4) == _lib.GOL_ERR_INVALID
    assert b"null batch" in lib.gol_last_error()
    assert list(out_b) == [71, 72, 73, 74] and list(out_s) == [75, 76, 77, 78]
    assert lib.gol_ensemble_set_rules(None, None, None, 0) == _lib.GOL_ERR_INVALID  # the null batch wins
    assert b"null batch" in lib.gol_last_error()
