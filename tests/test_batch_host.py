"""CPU tests of the batch handle's host side (include/gol/gol.h gol_batch_*): the geometry rule, the exported names in
every binding, and the host-only argument arithmetic under the sanitizers.  No kernel is launched here."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WIDTHS = (2, 3, 31, 32, 33, 100, 128, 129)
HEIGHTS = (2, 3, 64, 65, 100, 192, 255, 256, 257)


def _rule(w, h):
    """The fewest rows per lane in 1..4 that divide H with H / r <= 64, for W in 3..128 and H >= 3; 0 otherwise."""
    if not 3 <= w <= 128 or h < 3:
        return 0
    return next((r for r in (1, 2, 3, 4) if h % r == 0 and h // r <= 64), 0)


@pytest.mark.parametrize("w", WIDTHS)
def test_batch_supported_is_the_single_wave_rule(w):
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    for h in HEIGHTS:
        assert lib.gol_batch_supported(w, h) == _rule(w, h), (w, h)
        assert _lib.batch_supported(w, h) == _rule(w, h), (w, h)
    # spot values, so that a mistake shared by the rule above and the library still shows
    assert [lib.gol_batch_supported(100, h) for h in HEIGHTS] == [0, 1, 1, 0, 2, 3, 0, 4, 0]


def test_batch_is_exported():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import batch

    assert g.BoardBatch is batch.BoardBatch
    assert g.batch_supported(100, 100) == 2
    for name in ("set_cells", "get_cells", "seed_dotnet", "seed_splitmix", "clear", "step", "step_trace", "populations",
                 "hashes", "render_gray8", "generation", "close", "__enter__", "__exit__"):
        assert hasattr(g.BoardBatch, name), name


def _names(path, pattern=r"\b(gol_batch_\w+)\s*\("):
    src = open(os.path.join(ROOT, path)).read()
    return sorted(set(re.findall(pattern, src)))


def test_bindings_name_the_same_batch_functions():
    """The C header, the ctypes table, the F# P/Invoke module, the C++ mirror and the library's exports name one set of
    gol_batch_* functions (compared as name lists, by text)."""
    import ctypes

    from gameoflifewithactors_amd import _lib

    header = _names("include/gol/gol.h", r"(?m)^\s*int\s+(gol_batch_\w+)\s*\(")
    assert len(header) == 17 and "gol_batch_step_trace" in header and "gol_batch_supported" in header
    table = sorted(n for n in _lib.SIGNATURES if n.startswith("gol_batch_"))
    assert table == header
    fsharp = _names("bindings/fsharp/GolNative.fs", r"extern\s+\w+\s+(gol_batch_\w+)\s*\(")
    assert fsharp == header
    mirror = _names("include/gol/gol_host.hpp")
    assert set(mirror) <= set(header) and {"gol_batch_create", "gol_batch_step", "gol_batch_step_trace",
                                           "gol_batch_destroy"} <= set(mirror)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in header + ["gol_debug_batch_group_waves"]:
        assert hasattr(lib, name), name


def test_batch_host_arithmetic_under_sanitizers(tmp_path):
    """csrc/gol_batch_host.h (board ranges, trace lengths, the packed .NET seeding) compiled alone with the address and
    undefined-behaviour sanitizers (tests/cpp/test_batch_host.cpp, its own main): extreme int64 arguments, every
    refusal the header documents, and the seeded words against the byte order gol_seed_dotnet uses."""
    exe = tmp_path / "test_batch_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gameoflifewithactors_amd", "csrc"),
                    os.path.join(HERE, "cpp", "test_batch_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batch host ok" in r.stdout


def test_refusals_need_no_device():
    """Geometry and count are judged before the device is looked at: the codes are the same without a GPU."""
    import ctypes

    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    h = ctypes.c_void_p()
    for w, ht in ((129, 64), (128, 255), (100, 257)):
        assert lib.gol_batch_create(w, ht, 0, 4, ctypes.byref(h)) == _lib.GOL_ERR_UNSUPPORTED
        assert b"single-wave" in lib.gol_last_error() and not h.value
    for count in (0, -1, (1 << 22) + 1):
        assert lib.gol_batch_create(100, 100, 0, count, ctypes.byref(h)) == _lib.GOL_ERR_INVALID
        assert b"count" in lib.gol_last_error() and not h.value
    assert lib.gol_batch_create(2, 100, 0, 4, ctypes.byref(h)) == _lib.GOL_ERR_INVALID
    assert lib.gol_batch_create(100, 100, 7, 4, ctypes.byref(h)) == _lib.GOL_ERR_INVALID
    assert lib.gol_batch_step(None, 1) == _lib.GOL_ERR_INVALID
