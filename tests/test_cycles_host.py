"""CPU tests of the ensemble cycle census's host side (include/gol/gol.h gol_ensemble_cycles): the search's control flow
(csrc/gol_cycle_search.h, the code the kernel runs on a board in registers) against its definition on every small rho
sequence under the sanitizers, and the name in every binding.  No kernel is launched here."""
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_cycle_search_control_flow_under_sanitizers(tmp_path):
    """tests/cpp/test_cycle_search.cpp (its own main) with the address and undefined-behaviour sanitizers: for every
    transient 0..40, period 1..40 and budget G 1..90 the search resolves exactly when transient + period <= G, with
    the exact values, reports (-1, 0) otherwise, and never takes more than 6 G steps; the extremes of G = 2^20 too."""
    exe = tmp_path / "test_cycle_search"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "test_cycle_search.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cycle search ok: 147600 cases, 82820 resolved" in r.stdout  # 41 * 40 * 90; those with mu + lambda <= G


def test_the_search_header_has_no_hip():
    """The header is the CPU-checkable half of the kernel: nothing of HIP in it beyond the host/device attributes,
    and those only under __HIPCC__ (the sanitizer program above compiles it with plain g++)."""
    src = open(os.path.join(ROOT, "gameoflifewithactors_amd", "csrc", "gol_cycle_search.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "#include <hip" not in code and "__builtin_amdgcn" not in code and "threadIdx" not in code
    before, _, rest = code.partition("#if defined(__HIPCC__)")
    guarded, _, after = rest.partition("#endif")
    assert "__device__" in guarded and "__device__" not in before + after.replace("GOL_CYCLE_HD", "")
    body = open(os.path.join(ROOT, "gameoflifewithactors_amd", "csrc", "gol_batch_wave.h")).read()
    assert '#include "gol_cycle_search.h"' in body and "cycle_search<" in body
    kernel = open(os.path.join(ROOT, "gameoflifewithactors_amd", "csrc", "gol_cycles.hip")).read()
    assert '#include "gol_batch_wave.h"' in kernel and "board_census<" in kernel


def test_census_is_named_in_every_binding():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib, build

    name = "gol_ensemble_cycles"
    header = open(os.path.join(ROOT, "include", "gol", "gol.h")).read()
    assert re.search(r"(?m)^int\s+%s\s*\(gol_batch\*\s*b,\s*int64_t\s+max_generations," % name, header)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == 7
    fsharp = open(os.path.join(ROOT, "bindings", "fsharp", "GolNative.fs")).read()
    assert re.search(r"extern\s+int\s+%s\s*\(" % name, fsharp)
    assert name in open(os.path.join(ROOT, "include", "gol", "gol_host.hpp")).read()
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert callable(g.BoardBatch.cycles) and "transient" in g.BoardBatch.cycles.__doc__
    assert any(s.endswith("gol_cycles.hip") for s in build.SOURCES)
    assert any(h.endswith("gol_cycle_search.h") for h in build.HEADERS)


def test_census_refuses_a_null_batch_without_a_device():
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    out = [(ctypes.c_int64 * 4)(*([77] * 4)) for _ in range(4)]
    assert lib.gol_ensemble_cycles(None, 100, *out, 4) == _lib.GOL_ERR_INVALID
    assert b"null batch" in lib.gol_last_error()
    assert all(list(a) == [77] * 4 for a in out)
