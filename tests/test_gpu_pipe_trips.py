"""GPU parity of the level-pipelined pass's trip loops (csrc/gol_pipe.hip).

A stage runs its rows in trips of 4, in three loops: the fill's trips (nothing to hand on yet), the full trips (whole
rows in and out: no test of a row's range, the ring's half changed by one xor) and the last trip (any).  These are the
smallest shapes at which that split and the half's parity can go wrong: every residue of a stage's row count modulo 4
with an odd and an even number of trips, on a full strip and on packed remainder sub-strips, at both depths and with
one or two pipelines holding rows; several row groups with dozens of full trips and a short last group; bounded
boards every trip of which reaches outside the live rows; ghost-row strips whose first and last trips hold clamped
rows.  Bar: bit-exact against the oracle, and the pass's error word clear.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


def _pipe_errors():
    import ctypes

    from gameoflifewithactors_amd import _lib

    v = ctypes.c_int()
    assert _lib.load().gol_debug_pipe_errors(ctypes.byref(v)) == 0
    return v.value


def _rand(h, w, seed, p=0.4):
    return (np.random.default_rng(seed).random((h, w)) < p).astype(np.uint8)


def _run(gol, b0, k, gens, opts=None, boundary=0):
    h, w = b0.shape
    with gol.Board(w, h, boundary, tblock_k=k, ilv=4, options=dict(opts or {}, coop=0)) as b:
        assert (b.info()["tblock_k"], b.info()["ilv"]) == (k, 4)
        b.set_cells(b0).step(gens)
        return b.get_cells()


@pytest.mark.parametrize("split", [0, -1])  # the default shares (one pipeline holds all these rows: L = h); equal shares
@pytest.mark.parametrize("k", [16, 32])
@pytest.mark.parametrize("h", [41, 42, 43, 44, 45, 46])
@pytest.mark.parametrize("nblocks", [62, 64])  # one full strip; a strip and packed remainder sub-strips
def test_pipe_every_trip_count_residue(gol, oracle, nblocks, h, k, split):
    """L mod 4 = 0..3 on every stage (a stage reads L + 2K - 2sD rows, and 2D is a multiple of 4) with an odd and an
    even number of trips; three pipelined passes alternate the two buffers, then the streaming pass runs the rest."""
    w = 128 * nblocks
    b0 = _rand(h, w, nblocks * 1009 + h * 7 + k)
    gens = 3 * k + 3
    opts = {"pipe_split": split, "pipe_split2": split} if split else {}
    np.testing.assert_array_equal(_run(gol, b0, k, gens, opts), oracle.c_run(b0, gens, 0))
    assert _pipe_errors() == 0


@pytest.mark.parametrize("h", [517, 518])
def test_pipe_many_full_trips_over_several_groups(gol, oracle, h):
    """Several row groups, the last one short, and pipelines with dozens of full trips between their fill and their
    last trip."""
    w, k = 128 * 64, 32
    b0 = _rand(h, w, h)
    np.testing.assert_array_equal(_run(gol, b0, k, 2 * k), oracle.c_run(b0, 2 * k, 0))
    assert _pipe_errors() == 0


@pytest.mark.parametrize("h", [41, 42, 43, 44])
@pytest.mark.parametrize("nblocks", [64, 127])  # one strip with both edges; two edge strips and packed sub-strips
def test_pipe_bounded_every_trip_reaches_outside(gol, oracle, nblocks, h):
    """Fewer rows than the cone: every trip of every group zeroes rows outside the board, the last trip included, with
    live cells on the board's first and last rows."""
    w, k = 128 * nblocks, 32
    b0 = _rand(h, w, nblocks * 13 + h)
    b0[0, :] = 1
    b0[-1, ::2] = 1
    gens = 2 * k + 1
    np.testing.assert_array_equal(_run(gol, b0, k, gens, boundary=1), oracle.c_run(b0, gens, 1))
    assert _pipe_errors() == 0


@pytest.mark.parametrize("h", [125, 130])
def test_pipe_short_ghost_row_strips(gol, oracle, h):
    """3 ghost-row strips of 41 to 44 rows: the rows clamped into the buffer fall in the fill's and the last trips."""
    import torch

    from gameoflifewithactors_amd.strips import LocalBoard

    w, k = 128 * 64, 32
    b0 = _rand(h, w, 3 * h)
    gens = 2 * k + 8
    with LocalBoard(w, h, 0, k, 3, ilv=4) as lb:
        assert all(r.geom.ilv == 4 and r.geom.ghost == k for r in lb.runners)
        lb.set_cells(torch.as_tensor(b0))
        lb.step(gens)
        np.testing.assert_array_equal(lb.get_cells().numpy(), oracle.c_run(b0, gens, 0))
    assert _pipe_errors() == 0
