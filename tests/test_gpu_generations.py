"""GPU tests of Generations rules on the batch (BoardBatch(..., rule="B2/S/3") over gol_generations_create,
gol_generations_set_states / gol_generations_get_states; csrc/gol_batch_wave.h under the kernels of csrc/gol_batch.hip
and csrc/gol_cycles.hip): step, trace, state and cell I/O, the Gray8 frame, the stacked hash and the
cycle census at 2 to 8 states per cell.

The reference is tests/generations_reference.py (numpy, one board; pinned to tests/rule_reference.py at 2 states by
tests/test_generations_host.py).  count is 5 or 7, so the last workgroup of 4 waves is partly filled.
"""
import ctypes

import numpy as np
import pytest

import generations_reference as gref
import rule_reference as ref

pytestmark = pytest.mark.gpu

TORUS, BOUNDED = 0, 1
# every NW 1..4 and RPL 1..4, full and partial last words
SIZES = [(3, 3), (31, 64), (32, 100), (33, 192), (64, 256), (97, 12), (100, 100), (128, 8), (96, 192)]
NSTATES = (2, 3, 4, 5, 8)  # every plane count, both sides of each plane boundary
RULES = ("B2/S", "B2/S345", "B34/S12", "B3/S23", "B0123/S8")
ALL, BLINK = "B012345678/S012345678", "B012345678/S"


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


def _soups(w, h, n, seed=0):
    return np.stack([ref.soup(w, h, 9000 + 131 * w + h + seed + i) for i in range(n)])


def _states(w, h, n, nstates, seed=0):
    """Every state present (where the board has the cells for it)."""
    rng = np.random.default_rng(400 + 17 * w + h + nstates + seed)
    s = rng.integers(0, nstates, (n, h, w)).astype(np.uint8)
    flat = s.reshape(n, -1)
    for k in range(min(nstates, flat.shape[1])):
        flat[:, k] = k
    return s


def _run(states, rule, nstates, boundary, g):
    b, s = ref.masks(rule)
    return np.stack([gref.gen_step(x, b, s, nstates, boundary, g) for x in states])


def _check(b, want, nstates, oracle):
    got = b.get_states()
    wrong = sorted(set(np.argwhere(got != want)[:, 0].tolist()))
    assert not wrong, (wrong, np.argwhere(got != want)[:4].tolist())
    assert np.array_equal(b.get_cells(), (want == 1).astype(np.uint8))
    assert np.array_equal(b.populations(), (want == 1).sum((1, 2)))
    assert b.hashes().tolist() == [gref.gen_hash(x, nstates, oracle) for x in want]


def test_the_sizes_cover_every_words_per_row_and_rows_per_lane(gol):
    shapes = {((w + 31) // 32, gol.batch_supported(w, h)) for w, h in SIZES}
    assert {s[0] for s in shapes} == {1, 2, 3, 4} == {s[1] for s in shapes}
    assert any(w % 32 for w, _ in SIZES) and any(w % 32 == 0 for w, _ in SIZES)


# ------------------------------------------------------------------ 1. step against the reference, 2. split calls
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_step_equals_the_reference(gol, oracle, size, boundary):
    w, h = size
    for ni, nstates in enumerate(NSTATES):
        for ri in range(2):  # two of the five rules per (size, nstates); over the sizes every pair comes up
            rule = RULES[(SIZES.index(size) + 2 * ni + 3 * ri + boundary) % 5]
            count = 5 + 2 * ((ni + ri) % 2)
            start = _states(w, h, count, nstates, ri)
            with gol.BoardBatch(w, h, count, boundary, rule=rule, nstates=nstates) as b:
                assert b.nstates == nstates
                b.set_states(start)
                want, done = start, 0
                for g in (1, 2, nstates + 1, 37):
                    b.step(g - done)
                    want = _run(want, rule, nstates, boundary, g - done)
                    done = g
                    _check(b, want, nstates, oracle)
                    assert b.generation == g


def test_every_rule_meets_every_state_count():
    pairs = {(RULES[(si + 2 * ni + 3 * ri + bd) % 5], n) for si in range(len(SIZES)) for ni, n in enumerate(NSTATES)
             for ri in range(2) for bd in (0, 1)}
    assert pairs == {(r, n) for r in RULES for n in NSTATES}


@pytest.mark.parametrize("nstates", [3, 5, 8])
def test_split_calls_keep_the_decay_planes(gol, nstates):
    w, h = 100, 100
    start = _states(w, h, 5, nstates)
    with gol.BoardBatch(w, h, 5, TORUS, rule="B2/S345", nstates=nstates) as a, \
            gol.BoardBatch(w, h, 5, TORUS, rule="B2/S345", nstates=nstates) as b:
        a.set_states(start).step(3).step(0).step(5)
        b.set_states(start).step(8)
        assert a.generation == 8 == b.generation
        assert np.array_equal(a.get_states(), b.get_states())
        assert np.array_equal(a.get_states(), _run(start, "B2/S345", nstates, TORUS, 8))
        assert np.array_equal(a.step(0).get_states(), b.get_states())


# ------------------------------------------------------------------ 3. state I/O
@pytest.mark.parametrize("nstates", NSTATES)
def test_state_io(gol, nstates):
    from gameoflifewithactors_amd import _lib

    w, h = 33, 12
    start = _states(w, h, 7, nstates)
    assert set(np.unique(start).tolist()) == set(range(nstates))
    with gol.BoardBatch(w, h, 7, BOUNDED, rule="B2/S", nstates=nstates) as b:
        assert np.array_equal(b.set_states(start).get_states(), start)
        part = _states(w, h, 2, nstates, 5)
        b.step(2)
        assert b.generation == 2
        before = b.get_states()
        b.set_states(part, first=3)
        assert b.generation == 0
        want = before.copy()
        want[3:5] = part
        assert np.array_equal(b.get_states(), want)
        assert np.array_equal(b.get_states(4, 2), want[4:6])
        bad = part.copy()
        bad[1, h - 1, w - 1] = nstates
        b.step(1)
        held = b.get_states()
        with pytest.raises(ValueError):
            b.set_states(bad, first=0)
        assert b.generation == 1 and np.array_equal(b.get_states(), held)
        n = __import__("ctypes").c_int()
        _lib.check(b._lib.gol_generations_nstates(b._h, __import__("ctypes").byref(n)), "gol_generations_nstates")
        assert n.value == nstates


# ------------------------------------------------------------------ 4. setters clear dying cells
@pytest.mark.parametrize("nstates", [3, 4, 8])
def test_setters_of_cells_leave_no_dying_cell(gol, nstates):
    w, h = 97, 12
    start = _states(w, h, 5, nstates)
    cells = _soups(w, h, 2)
    with gol.BoardBatch(w, h, 5, TORUS, rule="B2/S", nstates=nstates) as b:
        b.set_states(start).set_cells(cells, first=1)
        want = start.copy()
        want[1:3] = cells
        assert np.array_equal(b.get_states(), want)  # the other boards keep their dying cells
        for seed in (lambda: b.seed_splitmix(11), lambda: b.seed_dotnet(np.arange(5)), lambda: b.clear()):
            b.set_states(start)
            assert b.get_states().max() == nstates - 1
            seed()
            assert np.array_equal(b.get_states(), b.get_cells()) and b.generation == 0
        assert b.get_states().max() == 0


def test_cell_setters_take_any_nonzero_byte_as_alive(gol, oracle):
    """set_cells on a Generations batch: a byte that is not zero is an alive cell, whatever its value -- a 2 or a 3 is
    no dying state -- and the boards it does not name keep theirs."""
    w, h, nstates = 33, 12, 4
    start = _states(w, h, 5, nstates)
    assert set(np.unique(start).tolist()) == set(range(nstates))
    cells = np.random.default_rng(71).choice(np.array([0, 1, 2, 3, 255], dtype=np.uint8), (2, h, w))
    assert all(set(np.unique(c).tolist()) == {0, 1, 2, 3, 255} for c in cells)
    want = start.copy()
    want[1:3] = cells != 0
    with gol.BoardBatch(w, h, 5, TORUS, rule="B2/S345", nstates=nstates) as b:
        got = b.set_states(start).set_cells(cells, first=1).get_states()
        assert np.array_equal(got[1:3], (cells != 0).astype(np.uint8)) and got[1:3].max() == 1
        assert np.array_equal(got[[0, 3, 4]], start[[0, 3, 4]])
        assert b.hashes().tolist() == [gref.gen_hash(x, nstates, oracle) for x in want]


def test_render_gray8_shows_the_alive_cells_alone(gol):
    """The Gray8 frame of a Generations board: alive_value at state 1, 0 at every other state; the bytes between a
    row's cells and the stride are 0, as tests/test_gpu_batch.py test_render_gray8 has them at 2 states."""
    from gameoflifewithactors_amd import _lib

    w, h, nstates, stride = 33, 12, 8, 40
    start = _states(w, h, 5, nstates)
    assert set(np.unique(start[3]).tolist()) == set(range(nstates))
    with gol.BoardBatch(w, h, 5, TORUS, rule="B2/S345", nstates=nstates) as b:
        b.set_states(start)
        pixels = np.full(stride * h, 7, dtype=np.uint8)
        ptr = pixels.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        _lib.check(b._lib.gol_batch_render_gray8(b._h, 3, ptr, stride, 200), "gol_batch_render_gray8")
        rows = pixels.reshape(h, stride)
        assert np.array_equal(rows[:, :w], np.where(start[3] == 1, 200, 0))
        assert not rows[:, w:].any()
        assert np.array_equal(b.get_states(), start)


# ------------------------------------------------------------------ 5. trace
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("nstates", [3, 5, 8])
def test_trace_counts_state_one_cells(gol, nstates, boundary):
    w, h = 100, 100
    start = _states(w, h, 7, nstates)
    with gol.BoardBatch(w, h, 7, boundary, rule="B34/S12", nstates=nstates) as b, \
            gol.BoardBatch(w, h, 7, boundary, rule="B34/S12", nstates=nstates) as plain:
        trace = b.set_states(start).step_trace(12, 3)
        assert trace.shape == (4, 7)
        want = start
        for t in range(4):
            want = _run(want, "B34/S12", nstates, boundary, 3)
            assert trace[t].tolist() == (want == 1).sum((1, 2)).tolist(), t
        assert np.array_equal(b.get_states(), want) and b.generation == 12
        assert np.array_equal(plain.set_states(start).step(12).get_states(), want)


# ------------------------------------------------------------------ 6. pad bits and outside cells
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_pad_bits_and_outside_cells_stay_dead(gol, size, boundary):
    w, h = size
    for nstates in (3, 8):
        with gol.BoardBatch(w, h, 5, boundary, rule=ALL, nstates=nstates) as b:
            b.set_cells(np.ones((5, h, w), dtype=np.uint8))
            for _ in range(20):
                assert b.step(1).populations().tolist() == [w * h] * 5
            b.set_rule(BLINK).set_cells(np.ones((5, h, w), dtype=np.uint8))
            trace = b.step_trace(2 * nstates + 1, 1)
            cycle = [0] * (nstates - 1) + [w * h]
            assert trace[:, 0].tolist() == (cycle * 3)[:2 * nstates + 1]
            assert (trace == trace[:, :1]).all()


# ------------------------------------------------------------------ 7. census
CENSUS = [  # rule, nstates, W, H, boundary, resolved at 64
    ("B2/S", 3, 16, 12, TORUS, 13),
    ("B2/S345", 4, 33, 9, BOUNDED, 14),
    ("B2/S3456", 6, 16, 12, TORUS, 4),
]


@pytest.mark.parametrize("case", CENSUS, ids=lambda c: "%s/%d" % c[:2])
def test_census_equals_brute_force(gol, case):
    rule, nstates, w, h, boundary, at64 = case
    birth, survive = ref.masks(rule)
    soups = np.stack([ref.soup(w, h, 1000 + i) for i in range(16)])
    with gol.BoardBatch(w, h, 16, boundary, rule=rule, nstates=nstates) as b:
        b.set_cells(soups)
        for budget in (512, 64):
            want = [gref.gen_cycles(x, birth, survive, nstates, boundary, budget) for x in soups]
            t, p, pop = b.cycles(budget)
            got = list(zip(t.tolist(), p.tolist(), pop.tolist()))
            assert got == want, budget
            resolved = sum(1 for x in got if x[0] >= 0)
            assert resolved == (16 if budget == 512 else at64)
            if budget == 512:
                periods, longest = {x[1] for x in got}, max(x[0] + x[1] for x in got)
                if nstates == 3:
                    assert periods == {1, 12, 16, 24, 192} and longest == 216
                elif nstates == 4:
                    assert periods == {1, 4, 12}
                else:
                    assert longest == 328
            assert np.array_equal(b.get_states(), soups) and b.generation == 0


def test_census_compares_the_dying_cells_too(gol):
    """Two boards with the same live cells and different dying cells are different boards: under B/S at 4 states a
    lone dying cell in state 2 is gone after 2 generations (transient 2), one in state 3 after 1."""
    s = np.zeros((5, 12, 16), dtype=np.uint8)
    s[1, 4, 4], s[2, 4, 4], s[3, 4, 4] = 2, 3, 1
    with gol.BoardBatch(16, 12, 5, TORUS, rule="B/S", nstates=4) as b:
        b.set_states(s)
        t, p, pop = b.cycles(16)
        assert list(zip(t.tolist(), p.tolist(), pop.tolist())) == [(0, 1, 0), (2, 1, 0), (1, 1, 0), (3, 1, 0), (0, 1, 0)]
        hs = b.hashes().tolist()
        assert len(set(hs[:4])) == 4 and hs[0] == hs[4]


# ------------------------------------------------------------------ 8. one rule per board
def test_one_rule_per_board_at_three_states(gol):
    w, h = 33, 12
    rules = ["B2/S", "B2/S345", "B34/S12", "B3/S23", "B0123/S8", "B36/S23", "B2/S3456"]
    soup = ref.soup(w, h, 77)
    start = np.stack([soup] * 7)
    with gol.BoardBatch(w, h, 7, TORUS, rule="B2/S/3") as b:
        b.set_rules(rules).set_cells(start)
        assert b.rules == [r + "/C3" for r in rules]
        b.step(9)
        want = np.stack([gref.gen_step(soup, *ref.masks(r), 3, TORUS, 9) for r in rules])
        assert np.array_equal(b.get_states(), want)
        b.set_cells(start)
        t, p, pop = b.cycles(256)
        got = list(zip(t.tolist(), p.tolist(), pop.tolist()))
        assert got == [gref.gen_cycles(soup, *ref.masks(r), 3, TORUS, 256) for r in rules]


# ------------------------------------------------------------------ 9. nstates = 2
def test_two_states_is_the_plain_batch(gol):
    w, h = 100, 100
    soups = _soups(w, h, 5)
    with gol.BoardBatch(w, h, 5, TORUS, rule="B36/S23", nstates=2) as a, gol.BoardBatch(w, h, 5, TORUS, rule="B36/S23") as b:
        assert a.nstates == 2 == b.nstates and a.rule == "B36/S23"
        a.set_states(soups).step(11)
        b.set_cells(soups).step(11)
        assert np.array_equal(a.get_cells(), b.get_cells()) and np.array_equal(a.get_states(), b.get_cells())
        assert a.hashes().tolist() == b.hashes().tolist()
        assert [x.tolist() for x in a.cycles(300)] == [x.tolist() for x in b.cycles(300)]


# ------------------------------------------------------------------ 10. interface
def test_interface(gol):
    for n in (1, 9):
        with pytest.raises(ValueError):
            gol.BoardBatch(16, 12, 5, TORUS, rule="B2/S", nstates=n)
    with pytest.raises(ValueError):
        gol.BoardBatch(16, 12, 5, TORUS, rule="B2/S/3", nstates=4)
    soups = _soups(16, 12, 5)
    with gol.BoardBatch(16, 12, 5, TORUS, rule="B2/S/3") as a, gol.BoardBatch(16, 12, 5, TORUS, rule="B2/S/C4") as b:
        assert (a.nstates, b.nstates) == (3, 4) and a.rule == "B2/S/C3" and b.rule == "B2/S/C4"
        with pytest.raises(ValueError):
            a.set_rule("B3/S23/4")
        assert a.rule == "B2/S/C3"
        assert a.set_rule("B3/S23").rule == "B3/S23/C3" and a.set_rule("b2/s/g3").rule == "B2/S/C3"
        assert a.rules == ["B2/S/C3"] * 5
        a.set_cells(soups).step(6)
        b.set_cells(soups).step(6)
        assert np.array_equal(a.get_states(), _run(soups, "B2/S", 3, TORUS, 6))
        assert np.array_equal(b.get_states(), _run(soups, "B2/S", 4, TORUS, 6))
