"""GPU parity of the level-pipelined pass where a stage's first level takes its block-edge words from LDS (the torus
kernels of csrc/gol_pipe.hip, lds_read_trip_edges).

At each stage's first level a lane's left and right neighbour words -- the left lane's last word and the right lane's
first -- are read from the LDS row next to the lane's own 16 bytes instead of from the neighbour lanes' registers.  A
wrong byte offset, a wrong row, or a halo lane's arbitrary word reaching a stored lane would show in the cells next to
a lane boundary (cells 127 and 128 of consecutive blocks), so the seeds put life there: half density, a live column
on each side of every lane boundary, and gliders crossing an inner lane boundary, the strip's halo lane (the board's
wrap) and the seam between the full strip and the remainder sub-strips.  Shapes: one full torus strip (62 blocks), a
strip plus packed remainder sub-strips (64 blocks: 16 sub-strips of 4 lanes, whose neighbours in the wave are other
sub-strips' halo lanes), both of 67 rows (the fill, full and last trips all run), and a pair of torus ghost-row
strips (the multi-GPU variant of the kernel).  K = 16 and 32 for K + 3 generations: one pipelined pass, then 3
generations of the streaming pass (DPP moves and life_next throughout), bit-exact against the oracle.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 67
GHOST_W, GHOST_H = 128 * 70, 900  # the torus ghost-row strips of tests/test_gpu_pipe.py
SEEDS = ["p50", "lane_boundary_columns", "gliders"]
SHAPES = {"strip_62_blocks": (128 * 62, ROWS), "strip_and_substrips_64_blocks": (128 * 64, ROWS),
          "ghost_row_strip_pair": (GHOST_W, GHOST_H)}


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
    if name == "p50":
        return (np.random.default_rng(5050 + w + h).random((h, w)) < 0.5).astype(np.uint8)
    b0 = np.zeros((h, w), np.uint8)
    if name == "lane_boundary_columns":  # cells 127 and 128 of consecutive blocks, every row
        b0[:, 127::128] = 1
        b0[:, 0::128] = 1
        return b0
    # gliders heading down and to the right, each already astride its boundary (columns x - 2 .. x): an inner lane
    # boundary, the board's wrap (the full strip's halo lanes) and, where the row has one, the strip / sub-strip seam;
    # at rows near the top, the middle (the ghost-row strips' seam) and the bottom
    glider = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], np.uint8)
    for x in sorted({128 * 31, 0, 128 * 62 % w}):
        for y in (5, h // 2 - 2, h - 8):
            for dy in range(3):
                for dx in range(3):
                    b0[y + dy, (x - 2 + dx) % w] = glider[dy, dx]
    return b0


_cases = {}


def _case(oracle, shape, seed, k):
    """(initial cells, the oracle's cells after k + 3 generations), computed once per case and left unchanged; the
    oracle goes on to generation 35 from the board it left at generation 19"""
    key = (shape, seed, k)
    if key not in _cases:
        if k == 32:
            b0, at19 = _case(oracle, shape, seed, 16)
            want = oracle.c_run(at19, 16, 0)
        else:
            w, h = SHAPES[shape]
            b0 = _seed(seed, h, w)
            want = oracle.c_run(b0, k + 3, 0)
        b0.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (b0, want)
    return _cases[key]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("k", [16, 32])
@pytest.mark.parametrize("shape", ["strip_62_blocks", "strip_and_substrips_64_blocks"])
def test_pipe_lds_edges_board_matches_oracle(gol, oracle, shape, k, seed):
    b0, want = _case(oracle, shape, seed, k)
    h, w = b0.shape
    with gol.Board(w, h, 0, tblock_k=k, ilv=4, options={"coop": 0}) as b:
        assert b.info()["tblock_k"] == k and b.info()["ilv"] == 4
        b.set_cells(b0).step(k + 3)
        got = b.get_cells()
    np.testing.assert_array_equal(got, want)
    assert _pipe_errors() == 0


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("k", [16, 32])
def test_pipe_lds_edges_ghost_row_strips_match_oracle(gol, oracle, k, seed):
    import torch

    from gameoflifewithactors_amd.strips import LocalBoard

    b0, want = _case(oracle, "ghost_row_strip_pair", seed, k)
    h, w = b0.shape
    with LocalBoard(w, h, 0, k, 2, ilv=4) as lb:
        assert all(r.geom.ilv == 4 and r.geom.ghost == k for r in lb.runners)
        lb.set_cells(torch.as_tensor(b0.copy()))
        lb.step(k + 3)
        got = lb.get_cells().numpy()
    np.testing.assert_array_equal(got, want)
    assert _pipe_errors() == 0
