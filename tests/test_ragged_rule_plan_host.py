"""CPU test of the ragged rows of the rule-generic and multi-plane streaming passes (csrc/gol_rule_plan.h "Ragged rows",
DESIGN.md 4.16): tests/cpp/test_ragged_rule_plan.cpp, a program of its own, under the address and undefined-behaviour
sanitizers, and what the kernels, the policy and the documents say about the passes.  No kernel is launched here."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gameoflifewithactors_amd", "csrc")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_ragged_rule_plan_under_sanitizers(tmp_path):
    """Every lane's window of every strip bit for bit against the brute-force ring (torus) or the row with zeros
    outside (bounded), every word index read inside the row (a heap row of exactly nw words), every (row, word) stored
    by exactly one lane, store and level masks the real cells: every width 64..4100 that is no multiple of 32 x heights
    {3, 7, 40} x K in {1, 2, 4, 8} x both boundaries x segment rows {planned, 5}."""
    exe = tmp_path / "test_ragged_rule_plan"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "cpp", "test_ragged_rule_plan.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    widths = sum(1 for w in range(64, 4101) if w % 32)
    assert f"ragged rule plan: {widths * 3 * 4 * 2 * 2} cases" in r.stdout and "ragged rule plan ok" in r.stdout


def test_the_kernels_call_the_plan_functions():
    for name in ("gol_rule_step.hip", "gol_gen_stream.hip"):
        kernel = _read(CSRC, name)
        for fn in ("rule_ragged_window(", "rule_ragged_load(", "rule_ragged_plain(", "rule_ragged_store_mask(",
                   "rule_ragged_level_mask("):
            assert fn in kernel, (name, fn)
    plan = re.sub(r"//[^\n]*", "", _read(CSRC, "gol_rule_plan.h"))
    assert "#include" not in plan.replace("#include <stdint.h>", "")  # the header still stands alone


def test_the_passes_are_named_values_beside_the_enumerator_list():
    board = _read(CSRC, "gol_board.h")
    assert "constexpr Pass kPassRuleRagged = static_cast<Pass>(13);" in board
    assert "constexpr Pass kPassGenRagged = static_cast<Pass>(14);" in board
    assert ("enum class Pass { None, Wave, Lanes, Coop, CoopRagged, Ring, StreamRagged, Resident, Bytes, Stream, Multi, "
            "RuleStream };") in board


def test_the_option_is_a_board_option_and_documented():
    assert '{"rule_ragged", 0,' in _read(CSRC, "gol_options.cpp")
    for doc in (("include", "gol", "gol.h"), ("INTEGRATION.md",), ("DESIGN.md",), ("README.md",)):
        assert "rule_ragged" in _read(ROOT, *doc), doc
    policy = _read(CSRC, "gol_policy.cpp")
    m = re.search(r"constexpr int64_t kRuleRaggedMinGens = (\d+);", policy)
    assert m and 4 <= int(m.group(1)) <= 16
    assert "4.16" in _read(ROOT, "DESIGN.md") and "ragged_rules_bench" in _read(ROOT, "tools", "README.md")
