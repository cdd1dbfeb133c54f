"""The shapes of tests/test_gpu_pipe_trips.py, planned on the host (no GPU): the level-pipelined pass's plan for each
of them covers the board (gol_debug_pipe_plan's host walk reports nothing bad), so what those tests try is the trip
loops and not a plan that was never meant to run."""
import ctypes

import pytest


def _bad(w, rows, ghost, wrap, boundary, k):
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    s = _lib.Strip(w, rows, 0, rows, ghost, w // 32, boundary, wrap, 4, 0)
    plan = (ctypes.c_int64 * 15)()
    assert lib.gol_debug_pipe_plan(ctypes.byref(s), k, 0, rows, 256, plan, 15) == 0, lib.gol_last_error()
    return plan[14], list(plan)


@pytest.mark.parametrize("k", [16, 32])
@pytest.mark.parametrize("h", [41, 42, 43, 44, 45, 46, 517, 518])
@pytest.mark.parametrize("nblocks", [62, 64])
def test_torus_shapes_plan(nblocks, h, k):
    bad, plan = _bad(128 * nblocks, h, 0, 1, 0, k)
    assert bad == 0, plan


@pytest.mark.parametrize("h", [41, 42, 43, 44])
@pytest.mark.parametrize("nblocks", [64, 127])
def test_bounded_shapes_plan(nblocks, h):
    bad, plan = _bad(128 * nblocks, h, 0, 0, 1, 32)
    assert bad == 0, plan


@pytest.mark.parametrize("rows", [41, 42, 43, 44])
def test_ghost_row_strip_shapes_plan(rows):
    bad, plan = _bad(128 * 64, rows, 32, 0, 0, 32)
    assert bad == 0, plan
