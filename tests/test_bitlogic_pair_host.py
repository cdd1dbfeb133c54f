"""CPU test of the row-pair form of the rule (pair_sum / life_next_pair in csrc/gol_bitlogic.h, the pipelined pass's 8
LUT ops per word and generation), compiled for the host.  No kernel is launched here."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pair_form_matches_life_next_on_host(tmp_path):
    """Both outputs of a row pair against life_next (and the reference rule, GameOfLifeLogic.fs:59-63) on all 2^12
    fillings of a 4 x 3 neighbourhood, and on random full words of a small interleaved torus stepped in row pairs with
    the pipelined pass's window rotation (tests/cpp/test_bitlogic_pair.cpp)."""
    exe = tmp_path / "test_bitlogic_pair"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(HERE, "cpp", "test_bitlogic_pair.cpp"), "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '"mismatches": 0' in r.stdout
