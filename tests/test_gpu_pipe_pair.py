"""GPU parity of the level-pipelined pass's row-pair rule (pair_sum / life_next_pair, csrc/gol_bitlogic.h; the trip
body of csrc/gol_pipe.hip) at the densities tests/test_gpu_pipe.py does not seed.

The pair form adds the two middle rows of a row pair's outputs once, as a 3-bit number, and its rule circuit relies on
two don't-cares: the pair's sum is never 7, and a live centre makes it at least 1.  Boards seeded at density 0.4 rarely
hold pair sums of 5-6, or a live centre in a nearly empty pair -- the cells next to those don't-cares -- so here the seeds
are sparse, half, dense, all alive, and a single live cell.  One full strip (torus: 62 blocks, bounded: 64 blocks with
the board's edges on the wave's outer lanes) of 67 rows -- fewer than the 2K-row cone at K = 32, an odd count, so the fill,
full and last trips all run -- for K + 3 generations: one pipelined pass, then 3 generations of the streaming pass
(life_next), bit-exact against the oracle.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 67
SEEDS = ["p10", "p50", "p90", "all_alive", "single_cell"]


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


def _pipe_errors():
    from gameoflifewithactors_amd import _lib

    v = ctypes.c_int()
    assert _lib.load().gol_debug_pipe_errors(ctypes.byref(v)) == 0
    return v.value


def _seed(name, h, w):
    if name == "all_alive":
        return np.ones((h, w), np.uint8)
    if name == "single_cell":
        b0 = np.zeros((h, w), np.uint8)
        b0[h // 2, w // 2 + 1] = 1
        return b0
    p = int(name[1:]) / 100.0
    return (np.random.default_rng(1000 + int(name[1:])).random((h, w)) < p).astype(np.uint8)


_cases = {}


def _case(oracle, boundary, seed, k):
    """(initial cells, the oracle's cells after k + 3 generations), computed once per case and left unchanged"""
    key = (boundary, seed, k)
    if key not in _cases:
        w = 128 * (64 if boundary else 62)
        b0 = _seed(seed, ROWS, w)
        want = oracle.c_run(b0, k + 3, boundary)
        b0.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (b0, want)
    return _cases[key]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("k", [16, 32])
@pytest.mark.parametrize("boundary", [0, 1], ids=["torus_62_blocks", "bounded_64_blocks"])
def test_pipe_pair_rule_matches_oracle(gol, oracle, boundary, k, seed):
    b0, want = _case(oracle, boundary, seed, k)
    h, w = b0.shape
    with gol.Board(w, h, boundary, tblock_k=k, ilv=4, options={"coop": 0}) as b:
        assert b.info()["tblock_k"] == k and b.info()["ilv"] == 4
        b.set_cells(b0).step(k + 3)
        got = b.get_cells()
    np.testing.assert_array_equal(got, want)
    assert _pipe_errors() == 0
