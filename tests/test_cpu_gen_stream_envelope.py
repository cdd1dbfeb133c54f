"""The register envelope of the multi-plane streaming pass as the compiler emits it (no GPU): csrc/gol_gen_stream.hip
compiled device-only with the build recipe's flags, each kernel's .vgpr_count and .private_segment_fixed_size read from
the listing's metadata.

gol_step runs, per (M, P, boundary), the deepest of K = 4, 2, 1 whose kernel has no scratch and at most 256 VGPRs, that
is at least two waves per SIMD (csrc/gol_gen_plan.h gen_stream_max_k).  That table is a condition on
the compiled kernels, so it is held against them here: every kernel without scratch, the chosen depth inside the
envelope, and the next deeper one outside it -- the table is the deepest that fits, not a guess.  Register counts only;
no instruction is looked for.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gameoflifewithactors_amd", "csrc")
DEPTHS, LAYOUTS, PLANES = (4, 2, 1), (1, 2, 4), (1, 2, 3)
MAX_VGPRS = 256


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(K, M, P, bounded): (vgprs, scratch bytes)} of every gol_gen_stream instantiation."""
    from gameoflifewithactors_amd import build

    out = str(tmp_path_factory.mktemp("gen_stream_listing") / "gol_gen_stream.s")
    subprocess.run([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only",
                    "-S", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, "gol_gen_stream.hip"),
                    "-o", out], check=True, timeout=600)
    text = open(out).read()
    found = {}
    # one metadata record per kernel: "- .agpr_count: ... .name: <symbol> ... .private_segment_fixed_size: n ...
    # .vgpr_count: n"; the records are split at their first key
    for rec in re.split(r"(?m)^  - \.agpr_count:", text)[1:]:
        name = re.search(r"(?m)^\s+\.name:\s+(\S+)", rec).group(1)
        m = re.search(r"gol_gen_streamILi(\d)ELi(\d)ELi(\d)ELb([01])E", name)
        if not m:
            continue
        k, lay, p, bounded = (int(x) for x in m.groups())
        vgprs = int(re.search(r"(?m)^\s+\.vgpr_count:\s+(\d+)", rec).group(1))
        scratch = int(re.search(r"(?m)^\s+\.private_segment_fixed_size:\s+(\d+)", rec).group(1))
        found[(k, lay, p, bool(bounded))] = (vgprs, scratch)
    return found


@pytest.fixture(scope="module")
def max_k(tmp_path_factory):
    """gen_stream_max_k as the library's host code has it: a small host program over csrc/gol_gen_plan.h."""
    d = tmp_path_factory.mktemp("gen_plan")
    src = d / "max_k.cpp"
    src.write_text('#include <stdio.h>\n#include <initializer_list>\n#include "gol_gen_plan.h"\nint main() {\n'
                   '    for (int m : {1, 2, 4}) for (int p = 1; p <= 3; p++) for (int b = 0; b < 2; b++)\n'
                   '        printf("%d %d %d %d\\n", m, p, b, gol::gen_stream_max_k(m, p, b != 0));\n    return 0;\n}\n')
    exe = d / "max_k"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    return {(m, p, bool(b)): k for m, p, b, k in (map(int, r.split()) for r in rows if r)}


def test_every_instantiation_is_there(kernels):
    assert set(kernels) == {(k, m, p, b) for k in DEPTHS for m in LAYOUTS for p in PLANES for b in (False, True)}
    for key, (vgprs, scratch) in sorted(kernels.items()):
        print("K=%d M=%d P=%d %-7s %3d VGPRs, %d B scratch" % (*key[:3], "bounded" if key[3] else "torus", vgprs, scratch))


def test_no_kernel_has_scratch(kernels):
    assert {key: v for key, v in kernels.items() if v[1] != 0} == {}


def test_the_table_names_an_instantiated_depth_that_fits(kernels, max_k):
    assert set(max_k) == {(m, p, b) for m in LAYOUTS for p in PLANES for b in (False, True)}
    for (m, p, b), k in max_k.items():
        assert k in DEPTHS, (m, p, b, k)
        vgprs, scratch = kernels[(k, m, p, b)]
        assert scratch == 0 and vgprs <= MAX_VGPRS, (m, p, b, k, vgprs, scratch)


def test_the_next_deeper_kernel_does_not_fit(kernels, max_k):
    deeper = 0
    for (m, p, b), k in max_k.items():
        if 2 * k >= 8:  # nothing deeper below 8
            continue
        vgprs, scratch = kernels[(2 * k, m, p, b)]
        assert vgprs > MAX_VGPRS or scratch > 0, (m, p, b, 2 * k, vgprs, scratch)
        deeper += 1
    assert deeper > 0  # the four-word layouts: the table decides something


def test_the_table_never_rises_with_the_planes(max_k):
    for m in LAYOUTS:
        for b in (False, True):
            ks = [max_k[(m, p, b)] for p in PLANES]
            assert ks == sorted(ks, reverse=True), (m, b, ks)
