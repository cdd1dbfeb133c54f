"""CPU test of the block forms of the row-pair rule (row_sum_block_staged / pair_sum_block / pair_g13_block /
pair_g2_block / pair_next_block in csrc/gol_bitlogic.h: the pipelined pass's LUTs stage by stage over a block's words),
compiled for the host.  No kernel is launched here."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pair_block_forms_match_word_forms_on_host(tmp_path):
    """Both outputs of a row pair by the block forms against life_next_pair, life_next and the reference rule
    (GameOfLifeLogic.fs:59-63) on all 2^12 fillings of a 4 x 3 neighbourhood centred in each of the block's words and
    across its edges, and on random full words at densities 0.1-1.0 for M = 4
    (tests/cpp/test_bitlogic_pair_block.cpp)."""
    exe = tmp_path / "test_bitlogic_pair_block"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(HERE, "cpp", "test_bitlogic_pair_block.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '"mismatches": 0' in r.stdout
