"""Which pass a gol_step call takes (csrc/gol_policy.cpp choose_pass), read back through the read-only debug option
"last_pass" (csrc/gol_debug.h), with the result of every call checked against the oracle.

One row per pass and per cut-over a call can cross: the single-wave pass (the reference's own 100 x 100 board,
GameOfLifeLogic.fs:5), the rows-on-lanes pass and its minimum call length, the cooperative pass, the LDS-resident and
streaming passes behind the "coop" and "resident_max_cells" options, the ragged boards' whole-word passes and their
minimum call lengths (kCoopRaggedMinGens 16, kStreamRaggedMinGens 4), and a multi-part board.  The expected values
were recorded from the dispatcher before it was split into choose_pass and one executor per pass.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the library's enum class Pass (csrc/gol_board.h); 0 = no step yet
NONE, WAVE, LANES, COOP, COOP_RAGGED, RING, STREAM_RAGGED, RESIDENT, BYTES, STREAM, MULTI = range(11)

TORUS, BOUNDED = 0, 1


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


def _rand(h, w, seed, p=0.4):
    return (np.random.default_rng(seed).random((h, w)) < p).astype(np.uint8)


# (w, h, boundary, options, Board keywords, generations, expected pass)
CASES = [
    (100, 100, TORUS, {}, {}, 10, WAVE),
    (128, 256, BOUNDED, {}, {}, 10, WAVE),
    (256, 256, BOUNDED, {}, {}, 100, LANES),
    (256, 256, BOUNDED, {}, {}, 10, COOP),  # fewer than 2 x the lanes depth (10)
    (2048, 2048, TORUS, {}, {}, 16, COOP),
    (256, 256, TORUS, {"coop": 0}, {}, 10, RESIDENT),
    (256, 256, TORUS, {"coop": 0, "resident_max_cells": 0}, {}, 10, STREAM),
    (8224, 4096, TORUS, {}, {}, 32, STREAM),  # wider than the cooperative pass's 8192
    (1001, 300, TORUS, {}, {}, 20, COOP_RAGGED),
    (1001, 300, TORUS, {}, {}, 3, BYTES),
    (200, 100, BOUNDED, {"resident_max_cells": 131072}, {}, 5, RESIDENT),
    (8209, 40, BOUNDED, {}, {}, 20, STREAM_RAGGED),
    (8209, 40, TORUS, {"ragged_ring": 2}, {}, 20, RING),
    (8209, 40, TORUS, {}, {}, 3, BYTES),
    (4096, 512, TORUS, {}, {"devices": [0, 0]}, 16, MULTI),
]


@pytest.mark.parametrize("w,h,boundary,options,kw,gens,want", CASES)
def test_pass_choice(gol, oracle, w, h, boundary, options, kw, gens, want):
    b0 = _rand(h, w, 1000 * boundary + w + h + gens)
    with gol.Board(w, h, boundary, options=options, **kw) as b:
        assert b.get_option("last_pass") == NONE
        b.set_cells(b0).step(gens)
        assert b.get_option("last_pass") == want
        np.testing.assert_array_equal(b.get_cells(), oracle.c_run(b0, gens, boundary))
        assert b.generation == gens
        assert b.get_option("last_pass") == want  # the readback changes nothing


def _canonical_words(cells):
    """The snapshot layout of gol_save_packed / gol_load_packed: row y is ceil(w / 64) uint64, bit i of word j = cell
    (64 j + i, y)."""
    h, w = cells.shape
    nc = (w + 63) // 64
    padded = np.zeros((h, nc * 64), np.uint8)
    padded[:, :w] = cells
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(h * nc)


SETTERS = ("set_cells", "load_packed", "seed_splitmix")


# the table's shapes; the 8224-wide board with 512 rows (its width picks the pass, asserted below; 4096 rows take 13 s)
DIRTY = [(w, 512 if w * h > 2**24 else h, *rest) for w, h, *rest in CASES]


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: f"{DIRTY[i][0]}x{DIRTY[i][1]}-pass{DIRTY[i][6]}-{SETTERS[i % 3]}")
def test_pass_choice_on_a_dirtied_handle(gol, oracle, case):
    """A board handle's buffers cannot be poisoned from outside, so they are dirtied from inside: every pass of the
    table first runs an all-ones board and then noise for the case's generations -- which leaves the ping-pong buffer,
    the ragged scratch rows, the ring copies and the hand-off granules holding another board -- before the board is
    overwritten (set_cells, load_packed or seed_splitmix, one per case) and stepped.  The result must be the oracle's
    and a fresh handle's: nothing of the earlier boards may reach it."""
    w, h, boundary, options, kw, gens, want = DIRTY[case]
    setter = SETTERS[case % 3]
    b0 = oracle.seed_splitmix(w, h, 77 + case) if setter == "seed_splitmix" else _rand(h, w, 5000 + case)
    with gol.Board(w, h, boundary, options=options, **kw) as fresh:
        fresh.set_cells(b0).step(gens)
        assert fresh.get_option("last_pass") == want
        fresh_hash, fresh_pop = fresh.hash(), fresh.population()
    with gol.Board(w, h, boundary, options=options, **kw) as b:
        b.set_cells(np.ones((h, w), np.uint8)).step(gens)
        assert b.get_option("last_pass") == want
        b.set_cells(_rand(h, w, 6000 + case, 0.5)).step(gens)
        assert b.get_option("last_pass") == want and b.generation == gens
        if setter == "set_cells":
            b.set_cells(b0)
        elif setter == "load_packed":
            b.load_packed(_canonical_words(b0))
        else:
            b.seed_splitmix(77 + case)
        assert b.generation == 0
        b.step(gens)
        assert b.get_option("last_pass") == want
        assert (b.hash(), b.population()) == (fresh_hash, fresh_pop)
        np.testing.assert_array_equal(b.get_cells(), oracle.c_run(b0, gens, boundary))
        assert b.generation == gens


def test_pass_choice_follows_the_call_length_on_a_ragged_board(gol, oracle):
    """The chooser meeting the ragged state: a long call leaves the board in the streaming pass's scratch rows, a short
    one brings the bytes up to date and steps them, the next long one packs them again."""
    w, h = 8209, 40
    cur = _rand(h, w, 11)
    with gol.Board(w, h, BOUNDED) as b:
        b.set_cells(cur)
        gen = 0
        for gens, want in ((20, STREAM_RAGGED), (3, BYTES), (20, STREAM_RAGGED)):
            b.step(gens)
            gen += gens
            cur = oracle.c_run(cur, gens, BOUNDED)
            assert b.get_option("last_pass") == want
            np.testing.assert_array_equal(b.get_cells(), cur, err_msg=f"generation {gen}")
            assert b.generation == gen


def test_last_pass_is_read_only(gol):
    with gol.Board(100, 100) as b:
        with pytest.raises(ValueError, match="read-only"):
            b.set_option("last_pass", 1)


@pytest.mark.parametrize("w,h,ok", [(100, 100, False), (256, 256, False), (2048, 2048, False), (8224, 4096, True)])
def test_pass_timing_takes_streaming_boards_only(gol, w, h, ok):
    """gol_pass_timing times one streaming pass, so it refuses the boards whose gol_step takes another one."""
    from gameoflifewithactors_amd import _lib

    with gol.Board(w, h, TORUS) as b:
        arrs = [(ctypes.c_double * 1)() for _ in range(3)]
        rc = b._lib.gol_pass_timing(b._h, 1, *arrs)
        assert rc == (_lib.GOL_OK if ok else _lib.GOL_ERR_UNSUPPORTED)
        assert b.generation == (b.info()["tblock_k"] if ok else 0)
