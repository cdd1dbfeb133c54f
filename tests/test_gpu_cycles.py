"""GPU tests of the ensemble cycle census (BoardBatch.cycles over gol_ensemble_cycles, csrc/gol_cycles.hip): for every
board of a batch the transient and the period of the cycle it runs into, found by one wavefront per board in one launch.

The reference is the definition, computed here: the CPU oracle steps a board one generation at a time (oracle.c_run) and
a dictionary keeps every board seen, up to G generations.  Values computed independently of it are pinned beside it, so
a mistake shared by the test and the library still shows.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TORUS, BOUNDED = 0, 1
GLIDER = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], np.uint8)
R_PENTOMINO = np.array([[0, 1, 1], [1, 1, 0], [0, 1, 0]], np.uint8)
UNRESOLVED = (-1, 0, 0)


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


def _rand(n, h, w, seed, p=0.4):  # the generator of test_gpu_batch.py
    return (np.random.default_rng(seed).random((n, h, w)) < p).astype(np.uint8)


def _census_one(oracle, b0, G, boundary):
    """(transient, period, population of B_transient) by the definition, or UNRESOLVED when t* > G."""
    seen = {np.packbits(b0).tobytes(): 0}
    pops = [int(b0.sum())]
    cur = b0
    for t in range(1, G + 1):
        cur = oracle.c_run(cur, 1, boundary)
        key = np.packbits(cur).tobytes()
        if key in seen:
            mu = seen[key]
            return (mu, t - mu, pops[mu])
        seen[key] = t
        pops.append(int(cur.sum()))
    return UNRESOLVED


_cache = {}


def _census(oracle, name, boards, G, boundary):
    """The reference of a named set of boards, computed once and shared by the tests that need it.  The boards are
    independent and the oracle's C step runs without the interpreter lock: eight at a time where a step is long enough
    to gain by it (on small boards the interpreter's own share dominates, and threads only contend for it)."""
    key = (name, G, boundary)
    if key not in _cache:
        oracle.c_oracle()  # loaded before the threads ask for it
        with ThreadPoolExecutor(8 if boards[0].size >= 4096 else 1) as pool:
            _cache[key] = list(pool.map(lambda b: _census_one(oracle, b, G, boundary), boards))
    return _cache[key]


def _got(result):
    return [tuple(int(a[i]) for a in result[:3]) for i in range(len(result[0]))]


PATTERNS = ("empty", "one cell", "block", "blinker", "glider", "row of 10", "R-pentomino")


def _patterns(h, w):
    b = np.zeros((len(PATTERNS), h, w), np.uint8)
    b[1, h // 2, w // 2] = 1
    b[2, 1:3, 1:3] = 1
    b[3, 5, 5:8] = 1
    b[4, 3:6, 1:4] = GLIDER  # heads south-east
    b[5, h // 2, (w - 10) // 2:(w - 10) // 2 + 10] = 1  # grows into the pentadecathlon
    b[6, h // 2:h // 2 + 3, w // 2:w // 2 + 3] = R_PENTOMINO
    return b


# computed apart from this file's reference; the torus values do not depend on where the pattern lies
PINNED = {
    ("glider", 33, 12, TORUS): (0, 528, 5),
    ("glider", 40, 12, TORUS): (0, 480, 5),
    ("glider", 100, 100, TORUS): (0, 400, 5),
    ("glider", 33, 12, BOUNDED): (27, 1, 4),
    ("glider", 100, 100, BOUNDED): (379, 1, 4),
    ("R-pentomino", 100, 100, TORUS): (1138, 2, 145),
    ("R-pentomino", 100, 100, BOUNDED): (1006, 2, 139),
}


@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("w,h", [(33, 12), (40, 12), (100, 100)])
def test_known_patterns(gol, oracle, w, h, boundary):
    G = 1500
    b0 = _patterns(h, w)
    want = _census(oracle, ("patterns", w, h), b0, G, boundary)
    with gol.BoardBatch(w, h, len(b0), boundary) as b:
        res = b.set_cells(b0).cycles(G)
    assert len(res) == 3 and all(a.shape == (len(b0),) and a.dtype == np.int64 for a in res)
    got = dict(zip(PATTERNS, _got(res)))
    print(w, h, boundary, got)
    assert got == dict(zip(PATTERNS, want))
    assert got["empty"] == (0, 1, 0) and got["one cell"] == (1, 1, 0)
    assert got["block"] == (0, 1, 4) and got["blinker"] == (0, 2, 3)
    assert got["row of 10"] == (2, 15, 18)
    for (name, pw, ph, pb), value in PINNED.items():
        if (pw, ph, pb) == (w, h, boundary):
            assert got[name] == value, name


def test_the_cap_is_exact(gol, oracle):
    """Resolved exactly when t* = transient + period <= G: the 33 x 12 torus glider (t* = 528) and the one-cell board
    (t* = 2), at G = t* and at G = t* - 1."""
    b0 = _patterns(12, 33)[[4, 1]]
    with gol.BoardBatch(33, 12, 2) as b:
        b.set_cells(b0)
        at = {G: _got(b.cycles(G)) for G in (528, 527, 2, 1)}
    print(at)
    assert at[528] == [(0, 528, 5), (1, 1, 0)]
    assert at[527] == [UNRESOLVED, (1, 1, 0)]
    assert at[2] == [UNRESOLVED, (1, 1, 0)]
    assert at[1] == [UNRESOLVED, UNRESOLVED]
    for G in at:
        assert at[G] == [_census_one(oracle, x, G, TORUS) for x in b0], G


# (w, h): (torus G, boards of the 8 the reference resolves at least), (bounded G, the same): NW 1..4, last-word bit 31
# and others, rows per lane 1..4, the 50-lane (100 x 100) and 64-lane cases
SWEEP = {
    (3, 3): ((50, 8), (50, 8)),
    (31, 5): ((100, 6), (100, 6)),
    (32, 64): ((700, 5), (400, 7)),
    (33, 12): ((200, 6), (200, 7)),
    (64, 100): ((2000, 4), (1500, 6)),
    (100, 100): ((2000, 5), (1200, 6)),
    (127, 192): ((2200, 3), (2000, 4)),
    (128, 256): ((2000, 1), (2400, 1)),
}


@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("w,h", list(SWEEP))
def test_geometry_sweep(gol, oracle, w, h, boundary):
    G, least = SWEEP[(w, h)][boundary]
    b0 = _rand(8, h, w, 1000 * w + h + boundary)
    want = _census(oracle, ("sweep", w, h), b0, G, boundary)
    resolved = [x for x in want if x != UNRESOLVED]
    assert len(resolved) >= least, want  # the test does not pass by leaving boards out
    if (w, h) != (3, 3):
        assert len(resolved) < 8, want
    if (w, h, boundary) == (31, 5, TORUS):
        assert any(mu + lam == G for mu, lam, _ in resolved), want  # one board lies exactly on the cap
    with gol.BoardBatch(w, h, 8, boundary) as b:
        b.set_cells(b0)
        res = b.cycles(G, with_steps=True)
        plain = b.cycles(G)
    steps = [int(s) for s in res[3]]
    print(w, h, boundary, G, _got(res), steps)
    assert _got(res) == want
    assert _got(plain) == want  # steps = NULL changes nothing
    assert all(0 < s <= 6 * G for s in steps), steps


def test_more_boards_than_simds(gol, oracle):
    """1100 boards on a chip of 1024 SIMDs, every one against the reference: a slip in the board index, or a wave that
    takes over a finished wave's slot with stale state, shows in some board."""
    n, w, h, G = 1100, 40, 12, 600
    b0 = _rand(n, h, w, 7)
    want = _census(oracle, "many", b0, G, TORUS)
    with gol.BoardBatch(w, h, n) as b:
        got = _got(b.set_cells(b0).cycles(G))
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, f"boards {bad[:10]} differ: {[(got[i], want[i]) for i in bad[:3]]}"
    assert 0 < sum(x == UNRESOLVED for x in want) < n


def test_read_only_and_current_cells(gol, oracle):
    """The census leaves cells, hashes and the generation counter alone, and starts from the boards as they are now:
    after step(10) a board with transient >= 10 reports 10 less with the same cycle, one with less reports 0."""
    w, h, G = 33, 12, 200
    b0 = np.concatenate([_patterns(h, w), _rand(8, h, w, 1000 * w + h + BOUNDED)])
    n = len(b0)
    want = _census(oracle, "current", b0, G, BOUNDED)
    with gol.BoardBatch(w, h, n, BOUNDED) as b:
        b.set_cells(b0).step(3)
        before = (b.get_cells(), b.hashes(), b.generation)
        b.cycles(G)
        assert np.array_equal(b.get_cells(), before[0]) and np.array_equal(b.hashes(), before[1])
        assert b.generation == before[2] == 3
        got0 = _got(b.set_cells(b0).cycles(G))
        assert got0 == want
        got10 = _got(b.step(10).cycles(G))
        assert b.generation == 10
        kinds = set()
        for i, (mu, lam, pop) in enumerate(want):
            if (mu, lam, pop) == UNRESOLVED:
                continue
            if mu >= 10:
                assert got10[i] == (mu - 10, lam, pop), i
            else:
                assert got10[i][:2] == (0, lam), i
                if lam == 1:
                    assert got10[i][2] == pop, i  # a still life is its own cycle
            kinds.add(mu >= 10)
        assert kinds == {True, False}, want
        # B_mu lies on a cycle of lambda generations: the hashes say so
        checked = 0
        for i, (mu, lam, pop) in enumerate(want):
            if (mu, lam, pop) == UNRESOLVED or checked == 4 or lam == 1 and mu == 0:
                continue
            b.set_cells(b0).step(mu)
            h_mu, p_mu = b.hashes()[i], b.populations()[i]
            assert b.step(lam).hashes()[i] == h_mu and p_mu == pop, i
            if mu > 0:  # ... and B_(mu-1) does not: the transient is no shorter
                b.set_cells(b0).step(mu - 1)
                h_prev = b.hashes()[i]
                assert b.step(lam).hashes()[i] != h_prev, i
            checked += 1
        assert checked == 4


def test_isolation(gol):
    """A glider board between two empty boards: the neighbours in memory report the empty board's (0, 1, 0)."""
    b0 = np.zeros((3, 12, 33), np.uint8)
    b0[1, 8:11, 29:32] = GLIDER  # crosses both seams of its torus
    with gol.BoardBatch(33, 12, 3) as b:
        got = _got(b.set_cells(b0).cycles(1500))
    assert got == [(0, 1, 0), (0, 528, 5), (0, 1, 0)]


def test_refusals(gol):
    """G outside 1..2^20, n != count or a NULL output: GOL_ERR_INVALID, the arrays untouched; steps = NULL is fine."""
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    n = 5
    b0 = _patterns(12, 33)[:n]
    with gol.BoardBatch(33, 12, n) as b:
        b.set_cells(b0).step(2)
        cells = b.get_cells()
        arrays = [np.full(n + 1, -77, np.int64) for _ in range(4)]
        t, p, pop, st = [a.ctypes.data_as(_lib.i64p) for a in arrays]
        for args in ((0, t, p, pop, st, n), (-1, t, p, pop, st, n), ((1 << 20) + 1, t, p, pop, st, n),
                     (100, t, p, pop, st, n - 1), (100, t, p, pop, st, n + 1), (100, None, p, pop, st, n),
                     (100, t, None, pop, st, n), (100, t, p, None, st, n)):
            assert lib.gol_ensemble_cycles(b._h, *args) == _lib.GOL_ERR_INVALID, args[0]
            assert lib.gol_last_error()
            assert all((a == -77).all() for a in arrays), args[0]
        for G in (0, (1 << 20) + 1):
            with pytest.raises(ValueError, match="max_generations"):
                b.cycles(G)
        assert lib.gol_ensemble_cycles(b._h, 100, t, p, pop, None, n) == _lib.GOL_OK
        assert (arrays[3] == -77).all() and all(a[n] == -77 for a in arrays)  # steps untouched, nothing past n
        assert lib.gol_ensemble_cycles(b._h, 1 << 20, t, p, pop, st, n) == _lib.GOL_OK  # the largest G is accepted
        assert [tuple(int(a[i]) for a in arrays[:3]) for i in range(n)] == _got(b.cycles(1 << 20))
        assert (arrays[3][:n] > 0).all() and (arrays[3][:n] <= 6 << 20).all()
        assert all(a[n] == -77 for a in arrays)
        assert b.generation == 2 and np.array_equal(b.get_cells(), cells)
