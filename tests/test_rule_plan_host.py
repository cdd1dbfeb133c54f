"""CPU test of the rule-generic streaming pass's plan (csrc/gol_rule_plan.h): tests/cpp/test_rule_plan.cpp, a program
of its own, under the address and undefined-behaviour sanitizers.  No kernel is launched here."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gameoflifewithactors_amd", "csrc")


def test_rule_plan_under_sanitizers(tmp_path):
    """Every (row, block) stored by exactly one (wave, lane), every loaded row and block inside the buffer or flagged
    not loaded, the wave count the launcher's: 1..200 blocks x heights 3..100 x K in {1, 2, 4, 8} x both boundaries x
    forced segment rows {0, 1, 5, 17}."""
    exe = tmp_path / "test_rule_plan"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "test_rule_plan.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rule plan: 627200 cases" in r.stdout and "rule plan ok" in r.stdout  # 200 x 98 x 4 x 2 x 4


def test_the_plan_header_has_no_hip_and_the_kernel_uses_it():
    src = open(os.path.join(CSRC, "gol_rule_plan.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("#include <hip", "__builtin_amdgcn", "threadIdx", "__global__", "hipError", "hipLaunch"):
        assert word not in code, word
    assert "#include" not in code.replace("#include <stdint.h>", "")  # and it stands alone
    kernel = open(os.path.join(CSRC, "gol_rule_step.hip")).read()
    for fn in ("rule_plan(", "rule_wave(", "rule_lane_load(", "rule_lane_store(", "rule_stream_grid("):
        assert fn in kernel, fn
