"""The level-pipelined pass's levels as the compiler emits them (no GPU): the device listing of csrc/gol_pipe.hip,
compiled with the build recipe's flags, read by tools/valu_dep_distance.py.

The pass is bound by VALU issue, and at 4 waves per SIMD a v_bitop3 that issues 2 or 3 instructions behind the one that
wrote its source is 7-12 % slower than one 8 or more behind (DESIGN.md 4.7 "dependent distance").  The staged order of
a level (gol_bitlogic.h pair_sum_block and the block forms beside it) exists to keep the rule's LUTs away from their
producers; nothing but the listing shows whether the compiler kept it.  So: the instruction counts of a trip are what
they were, the register envelope still gives 4 waves per SIMD, the levels hold no instruction that would shift the
address parity of the ones after it, and in the K = 32 torus kernel's full-trips loop no v_bitop3 is 2 or 3 behind its
producer (the parent had 42.6 % of them there, profiles/pipe_dep_distance/dist_parent.txt).
"""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gameoflifewithactors_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "valu_dep_distance.py")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from gameoflifewithactors_amd import build

    out = str(tmp_path_factory.mktemp("pipe_listing") / "gol_pipe.s")
    subprocess.run([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only",
                    "-S", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, "gol_pipe.hip"), "-o", out],
                   check=True, timeout=600)
    return out


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("valu_dep_distance", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels(listing, tool):
    with open(listing) as f:
        res = tool.analyse(f.read())
    assert len(res) == 6, list(res)  # K = 16 and 32: torus, ghost-row strips, bounded
    return res


def test_tool_prints_every_kernel_and_loop(listing, kernels):
    import sys

    r = subprocess.run([sys.executable, TOOL, listing], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for name in kernels:
        assert name in r.stdout
    assert r.stdout.count("full trips: v_bitop3_b32 512, v_alignbit_b32 32") == 6


def test_trip_instruction_counts_unchanged(kernels):
    for name, k in kernels.items():
        dpp = 32 if "bounded" in name else 24  # a torus stage's first level takes its block-edge words from LDS
        for loop in ("full trips", "last trip"):
            assert k["loops"][loop]["counts"] == {"v_bitop3_b32": 512, "v_alignbit_b32": 32, "v_mov_b32_dpp": dpp}, (name, loop)


def test_register_envelope(kernels):
    for name, k in kernels.items():
        e = k["envelope"]
        assert e["vgprs"] is not None and e["vgprs"] <= 128, (name, e)
        assert e["scratch"] == 0 and e["occupancy"] == 4, (name, e)


def test_no_other_instruction_inside_the_torus_levels(kernels):
    """every instruction of a level is 8 bytes long: level_align() pins the first, a 4-byte one would unpin the rest"""
    for name, k in kernels.items():
        if "bounded" in name:  # their edge trips branch inside the levels, as before
            continue
        for loop in ("full trips", "last trip"):
            assert k["loops"][loop]["inside"] == {}, (name, loop)


def test_no_lut_two_or_three_behind_its_producer(kernels, tool):
    name = next(n for n in kernels if n.startswith("K=32 torus"))
    hist = kernels[name]["loops"]["full trips"]["total"]["v_bitop3_b32"]
    assert sum(hist.values()) == 512
    assert hist[2] == 0 and hist[3] == 0, dict(hist)
    assert tool.share(hist, (2, 3)) == 0.0
