"""GPU parity of the level-pipelined pass with its levels in staged order (csrc/gol_pipe.hip: each LUT of the row-pair
circuit for a block's four words at a time, gol_bitlogic.h pair_sum_block / pair_g13_block / pair_g2_block /
pair_next_block, with the other row's sum and a row move between g2 and next; DESIGN.md 4.7 "dependent distance").

The order changes which value is live where -- the first output's words must not replace the row they are the centre
of before the second output has read it, the carried sums must move on after both outputs, the row move taken as
filler must read the first output and not the row it replaces -- and a slip shows as wrong cells, not as a fault.  The
smallest shapes that reach every stage branch and all three trip loops (fill, full, last), each of 67 rows -- fewer
than the 2K-row cone at K = 32, and odd:
  one full torus strip (62 blocks); a torus strip plus packed remainder sub-strips (64 blocks); a bounded board of one
  strip with both edges on the wave's outer lanes (64 blocks); a pair of torus ghost-row strips (the multi-GPU variant).
K = 16 and 32 for K + 3 generations: one pipelined pass, then 3 generations of the streaming pass (life_next).  Seeds at
the densities next to the pair circuit's don't-cares (tests/test_gpu_pipe_pair.py): sparse, half, dense, all alive, one
live cell.  Every result cell for cell against the CPU oracle.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 67
SEEDS = ["p10", "p50", "p90", "all_alive", "single_cell"]
# name: (width, height, boundary, ghost-row strips)
SHAPES = {
    "torus_strip_62_blocks": (128 * 62, ROWS, 0, 0),
    "torus_strip_and_substrips_64_blocks": (128 * 64, ROWS, 0, 0),
    "bounded_64_blocks": (128 * 64, ROWS, 1, 0),
    "ghost_row_strip_pair": (128 * 64, 2 * ROWS, 0, 2),
}


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
    return (np.random.default_rng(2000 + int(name[1:])).random((h, w)) < p).astype(np.uint8)


_cases = {}


def _case(oracle, shape, seed, k):
    """(initial cells, the oracle's cells after k + 3 generations), computed once per case and left unchanged"""
    key = (shape, seed, k)
    if key not in _cases:
        w, h, boundary, _ = SHAPES[shape]
        b0 = _seed(seed, h, w)
        want = oracle.c_run(b0, k + 3, boundary)
        b0.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (b0, want)
    return _cases[key]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("k", [16, 32])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pipe_staged_levels_match_oracle(gol, oracle, shape, k, seed):
    b0, want = _case(oracle, shape, seed, k)
    h, w = b0.shape
    _, _, boundary, strips = SHAPES[shape]
    if strips:
        import torch

        from gameoflifewithactors_amd.strips import LocalBoard

        with LocalBoard(w, h, 0, k, strips, ilv=4) as lb:
            assert all(r.geom.ilv == 4 and r.geom.ghost == k for r in lb.runners)
            lb.set_cells(torch.as_tensor(b0.copy()))
            lb.step(k + 3)
            got = lb.get_cells().numpy()
    else:
        with gol.Board(w, h, boundary, tblock_k=k, ilv=4, options={"coop": 0}) as b:
            assert b.info()["tblock_k"] == k and b.info()["ilv"] == 4
            b.set_cells(b0).step(k + 3)
            got = b.get_cells()
    np.testing.assert_array_equal(got, want)
    assert _pipe_errors() == 0
