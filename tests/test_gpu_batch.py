"""GPU tests of the batch handle (BoardBatch over gol_batch_*, csrc/gol_batch.hip): many small boards, one wavefront per
board, stepped by one launch.  Everything is compared exactly with the CPU oracle (oracle.c_run, board_hash, population,
c_seed_dotnet, c_seed_splitmix, render_gray8); the boards of a batch are seeded differently, so an index mix-up shows.
"""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TORUS, BOUNDED = 0, 1
GLIDER = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], np.uint8)


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


def _rand(n, h, w, seed, p=0.4):
    return (np.random.default_rng(seed).random((n, h, w)) < p).astype(np.uint8)


def _run(oracle, boards, gens, boundary):
    return np.stack([oracle.c_run(b, gens, boundary) for b in boards])


# NW 1..4, last-word bit 31 and others, rows per lane 1..4, the 50-lane (100 x 100) and 64-lane cases
SHAPES = [(3, 3), (31, 5), (32, 64), (33, 12), (64, 100), (100, 100), (127, 192), (128, 256)]


@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("w,h", SHAPES)
def test_geometry_sweep(gol, oracle, w, h, boundary):
    b0 = _rand(5, h, w, 1000 * w + h)
    with gol.BoardBatch(w, h, 5, boundary) as b:
        assert b.info() == {"width": w, "height": h, "boundary": boundary, "count": 5,
                            "rows_per_lane": gol.batch_supported(w, h)}
        b.set_cells(b0).step(70)
        assert b.generation == 70
        got = b.get_cells()
    want = _run(oracle, b0, 70, boundary)
    for i in range(5):
        assert np.array_equal(got[i], want[i]), f"board {i}"


def test_more_boards_than_simds(gol, oracle):
    """1100 boards on a chip of 1024 SIMDs: a surplus wave, or a slip in the board index, shows in some board."""
    n, w, h, gens = 1100, 40, 12, 40
    b0 = _rand(n, h, w, 7)
    with gol.BoardBatch(w, h, n) as b:
        got = b.set_cells(b0).step(gens).get_cells()
    want = _run(oracle, b0, gens, TORUS)
    bad = [i for i in range(n) if not np.array_equal(got[i], want[i])]
    assert not bad, f"boards {bad[:10]} differ"


@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
def test_isolation(gol, oracle, boundary):
    """A glider in the middle board of three crosses both seams of its torus (or ends at the edge of its bounded
    board, as the oracle says); the boards on either side of it in memory stay empty."""
    w, h = 33, 12
    b0 = np.zeros((3, h, w), np.uint8)
    b0[1, 8:11, 29:32] = GLIDER  # heads south-east: over the right and the bottom edge within 100 generations
    want = oracle.c_run(b0[1], 100, boundary)
    if boundary == TORUS:
        assert oracle.population(want) == 5 and not np.array_equal(want, b0[1])
    with gol.BoardBatch(w, h, 3, boundary) as b:
        got = b.set_cells(b0).step(100).get_cells()
        pops = b.populations()
    assert not got[0].any() and not got[2].any()
    assert np.array_equal(got[1], want)
    assert list(pops) == [0, oracle.population(want), 0]


def test_calls_compose(gol, oracle):
    b0 = _rand(4, 100, 100, 11)
    with gol.BoardBatch(100, 100, 4) as a, gol.BoardBatch(100, 100, 4) as b:
        a.set_cells(b0).step(7).step(0).step(25)
        b.set_cells(b0).step(32)
        assert a.generation == 32 and b.generation == 32
        ga, gb = a.get_cells(), b.get_cells()
    assert np.array_equal(ga, gb)
    assert np.array_equal(ga, _run(oracle, b0, 32, TORUS))


@pytest.fixture(scope="module")
def curves(oracle):
    """Per-generation populations and final boards of the trace tests' batches, computed once: {(w, h, boundary):
    (initial boards, populations after generation 1..60 as (60, 5), boards after 60)}."""
    out = {}
    for (w, h), boundary in (((100, 100), TORUS), ((33, 12), TORUS), ((33, 12), BOUNDED)):
        b0 = _rand(5, h, w, 31 * w + boundary)
        pops = np.zeros((60, 5), np.uint32)
        cur = [b for b in b0]
        for g in range(60):
            cur = [oracle.c_run(c, 1, boundary) for c in cur]
            pops[g] = [oracle.population(c) for c in cur]
        out[(w, h, boundary)] = (b0, pops, np.stack(cur))
    return out


@pytest.mark.parametrize("every", [1, 15])
@pytest.mark.parametrize("w,h,boundary", [(100, 100, TORUS), (33, 12, TORUS), (33, 12, BOUNDED)])
def test_trace(gol, curves, w, h, boundary, every):
    """33 x 12 runs on 12 of the wave's 64 lanes: what the other 52 hold must not reach the sums."""
    b0, pops, final = curves[(w, h, boundary)]
    with gol.BoardBatch(w, h, 5, boundary) as b, gol.BoardBatch(w, h, 5, boundary) as plain:
        trace = b.set_cells(b0).step_trace(60, every)
        assert trace.shape == (60 // every, 5) and trace.dtype == np.uint32
        assert np.array_equal(trace, pops[every - 1::every])
        assert b.generation == 60
        got = b.get_cells()
        assert np.array_equal(got, final)
        assert np.array_equal(got, plain.set_cells(b0).step(60).get_cells())
        # a traced call of no generations is a no-op with an empty trace
        assert np.array_equal(b.step_trace(0, every), np.zeros((0, 5), np.uint32))
        assert b.generation == 60


def test_workgroup_shapes_agree(gol, curves):
    """Four boards per 256-thread workgroup (the A/B shape of DESIGN.md 4.9; 5 boards leave three surplus waves in the
    second group) gives what one board per 64-thread workgroup gives, trace included."""
    from gameoflifewithactors_amd import _lib

    b0, pops, final = curves[(33, 12, BOUNDED)]
    with gol.BoardBatch(33, 12, 5, BOUNDED) as b:
        _lib.check(_lib.load().gol_debug_batch_group_waves(b._h, 4))
        assert _lib.load().gol_debug_batch_group_waves(b._h, 2) == _lib.GOL_ERR_INVALID
        assert np.array_equal(b.set_cells(b0).step_trace(60, 1), pops)
        assert np.array_equal(b.get_cells(), final)
        assert np.array_equal(b.set_cells(b0).step(60).get_cells(), final)


def test_trace_refuses_a_ragged_sampling(gol):
    from gameoflifewithactors_amd import _lib

    b0 = _rand(5, 12, 33, 3)
    with gol.BoardBatch(33, 12, 5) as b:
        b.set_cells(b0).step(3)
        with pytest.raises(ValueError, match="multiple of every"):
            b.step_trace(60, 7)
        buf = (ctypes.c_uint32 * 64)()
        lib = _lib.load()
        assert lib.gol_batch_step_trace(b._h, 60, 7, buf, 40) == _lib.GOL_ERR_INVALID
        assert lib.gol_batch_step_trace(b._h, 60, 0, buf, 40) == _lib.GOL_ERR_INVALID
        assert lib.gol_batch_step_trace(b._h, 60, 15, buf, 19) == _lib.GOL_ERR_INVALID  # wrong len
        assert lib.gol_batch_step_trace(b._h, 1 << 40, 1, buf, (1 << 40) * 5) == _lib.GOL_ERR_INVALID  # > 2^26 entries
        assert b.generation == 3
        with gol.BoardBatch(33, 12, 5) as ref:
            assert np.array_equal(b.get_cells(), ref.set_cells(b0).step(3).get_cells())


@pytest.mark.parametrize("w,h", [(100, 100), (33, 12), (64, 100), (128, 256)])
def test_observables(gol, oracle, w, h):
    """populations() and hashes() per board: the oracle's, and those of a single Board holding the same cells (a byte
    board for the ragged widths, a packed one for 64 and 128)."""
    b0 = _rand(6, h, w, 5 * w + h, p=0.3)
    b0[4] = 0
    with gol.BoardBatch(w, h, 6) as b:
        b.set_cells(b0).step(9)
        cells, pops, hashes = b.get_cells(), b.populations(), b.hashes()
    assert pops.dtype == np.int64 and hashes.dtype == np.uint64
    for i in range(6):
        want = oracle.c_run(b0[i], 9, TORUS)
        assert np.array_equal(cells[i], want)
        assert int(pops[i]) == oracle.population(want), i
        assert int(hashes[i]) == oracle.board_hash(want), i
        with gol.Board(w, h) as single:
            single.set_cells(cells[i])
            assert single.info()["packed"] == (w % 32 == 0)
            assert (single.population(), single.hash()) == (int(pops[i]), int(hashes[i])), i


def test_set_get_round_trip_and_ranges(gol):
    w, h = 33, 12
    b0 = _rand(6, h, w, 21)
    with gol.BoardBatch(w, h, 6) as b:
        assert not b.get_cells().any()  # a new batch is all dead
        b.set_cells(b0).step(4)
        assert b.generation == 4
        assert np.array_equal(b.set_cells(b0).get_cells(), b0)  # no stepping in between
        assert b.generation == 0  # the setters reset the counter
        new = _rand(2, h, w, 22)
        b.set_cells(new, first=2)
        got = b.get_cells()
        for i in (0, 1, 4, 5):
            assert np.array_equal(got[i], b0[i]), i
        assert np.array_equal(got[2:4], new)
        assert np.array_equal(b.get_cells(3, 2), got[3:5])
        assert np.array_equal(b.get_cells(5), got[5:])
        b.set_cells(b0[0], first=5)  # a single (H, W) board
        assert np.array_equal(b.get_cells(5, 1)[0], b0[0])
        b.clear()
        assert not b.get_cells().any() and b.generation == 0


@pytest.mark.parametrize("mode", [0, 1])
def test_seed_dotnet(gol, oracle, mode):
    seeds = [0, 1, 42]
    with gol.BoardBatch(100, 100, 3) as b:
        b.step(2)
        got = b.seed_dotnet(seeds, mode).get_cells()
        assert b.generation == 0
        with pytest.raises(ValueError):
            b.seed_dotnet([0, 1], mode)
        with pytest.raises(ValueError):
            b.seed_dotnet(seeds, 2)
    for i, s in enumerate(seeds):
        assert np.array_equal(got[i], oracle.c_seed_dotnet(100, 100, s, mode)), s


@pytest.mark.parametrize("w,h", [(100, 100), (33, 12), (128, 256)])
def test_seed_splitmix(gol, oracle, w, h):
    s = 0x5EED
    with gol.BoardBatch(w, h, 4) as b:
        got = b.seed_splitmix(s).get_cells()
    for i in range(4):
        assert np.array_equal(got[i], oracle.c_seed_splitmix(w, h, s + i)), i


def test_render_gray8(gol, oracle):
    w, h = 33, 12
    b0 = _rand(3, h, w, 8)
    with gol.BoardBatch(w, h, 3) as b:
        b.set_cells(b0)
        assert np.array_equal(b.render_gray8(1, alive_value=128, stride=w + 3),
                              oracle.render_gray8(b0[1], 128, w + 3))
        assert np.array_equal(b.render_gray8(2, alive_value=255), oracle.render_gray8(b0[2], 255))
        with pytest.raises(ValueError):
            b.render_gray8(3)
        with pytest.raises(ValueError):
            b.render_gray8(0, stride=w - 1)


def test_refusals(gol, oracle):
    """Every refusal returns before any device work, with a message; a batch created afterwards works."""
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    h = ctypes.c_void_p()
    for w, ht in ((129, 64), (128, 255), (100, 257)):
        assert lib.gol_batch_create(w, ht, TORUS, 3, ctypes.byref(h)) == _lib.GOL_ERR_UNSUPPORTED
        assert lib.gol_last_error() and not h.value
        with pytest.raises(NotImplementedError):
            gol.BoardBatch(w, ht, 3)
    assert lib.gol_batch_create(100, 100, TORUS, 0, ctypes.byref(h)) == _lib.GOL_ERR_INVALID
    assert b"count" in lib.gol_last_error() and not h.value
    b0 = _rand(6, 12, 33, 9)
    with gol.BoardBatch(33, 12, 6) as b:
        b.set_cells(b0)
        buf = np.zeros(6 * 12 * 33 + 8, np.uint8)
        p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        n1 = 12 * 33
        for first, n, length in ((5, 2, 2 * n1), (-1, 1, n1), (6, 1, n1), (0, 7, 7 * n1), (0, 0, 0),  # ranges
                                 (2, 2, 2 * n1 - 1), (2, 2, 2 * n1 + 1), (0, 6, n1)):                 # lengths
            for fn in (lib.gol_batch_set_cells, lib.gol_batch_get_cells):
                assert fn(b._h, first, n, p, length) == _lib.GOL_ERR_INVALID, (first, n, length)
                assert b"first" in lib.gol_last_error()
        out64 = (ctypes.c_int64 * 8)()
        assert lib.gol_batch_populations(b._h, out64, 5) == _lib.GOL_ERR_INVALID
        assert lib.gol_batch_step(b._h, -1) == _lib.GOL_ERR_INVALID
        assert not buf.any()
        assert np.array_equal(b.get_cells(), b0)  # nothing was written
    with gol.BoardBatch(33, 12, 6) as b:
        assert np.array_equal(b.set_cells(b0).step(5).get_cells(), _run(oracle, b0, 5, TORUS))


def test_config1_through_the_batch(gol):
    """BASELINE config 1 (the reference's 100 x 100 torus, seeds 0, 1 and 42) as one batch of three, walked to the
    fixtures' checkpoints and compared as test_gpu_parity.py compares them for a single board."""
    with open(os.path.join(HERE, "golden", "golden_small.json")) as f:
        cases = json.load(f)["cases"]
    names = ["c1_torus100_dotnetmod2_seed0", "c1_torus100_dotnetmod2_seed1", "c1_torus100_dotnetmod2_seed42"]
    boards = np.load(os.path.join(HERE, "golden", "golden_boards.npz"))
    for name in names:
        c = cases[name]
        assert (c["width"], c["height"], c["boundary"], c["init"]) == (100, 100, "torus", "dotnet-mod2")
    checkpoints = sorted(int(c) for c in cases[names[0]]["checkpoints"])
    assert all(sorted(int(c) for c in cases[n]["checkpoints"]) == checkpoints for n in names)
    with gol.BoardBatch(100, 100, 3) as b:
        b.seed_dotnet([cases[n]["seed"] for n in names], gol.INIT_DOTNET_MOD2)
        done = compared = 0
        for cp in checkpoints:
            b.step(cp - done)
            done = cp
            hashes, pops, cells = b.hashes(), b.populations(), b.get_cells()
            for i, name in enumerate(names):
                want = cases[name]["checkpoints"][str(cp)]
                assert str(int(hashes[i])) == want["hash"], f"{name} gen {cp}"
                assert int(pops[i]) == want["population"], f"{name} gen {cp}"
                key = f"{name}_g{cp}"
                if key in boards.files:
                    assert np.array_equal(np.packbits(cells[i], axis=None, bitorder="little"), boards[key]), key
                    compared += 1
        assert b.generation == checkpoints[-1] and compared == 6
