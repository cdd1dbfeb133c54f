"""GPU tests of life-like rules on the batch (BoardBatch(rule=...), set_rule over gol_ensemble_set_rule; the rule-table
kernels of csrc/gol_batch.hip and csrc/gol_cycles.hip): step, population trace and cycle census under
any B.../S... rule.

The reference is the definition, computed here in numpy and vectorised over the batch axis: eight np.roll on a torus, a
zero-padded window on a bounded board (the cells outside are dead and are no cells of the board, also under B0), then
birth[n] / survive[n] looked up per cell.  tests/test_rule_host.py ties it, under B3/S23, to the CPU oracle every other
test is checked against.  Its census is test_gpu_cycles.py's dictionary search over it.  Outcomes computed apart from
this reference are pinned beside it, so a mistake shared by the test and the library still shows.
"""
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TORUS, BOUNDED = 0, 1
UNRESOLVED = (-1, 0, 0)

# (W, H, boards): the smallest geometry that reaches each code shape
GEOMETRIES = [
    (3, 3, 32),      # NW 1, RPL 1; every neighbour is another cell of the torus
    (32, 64, 32),    # last bit 31, all 64 lanes
    (33, 12, 32),    # NW 2, ragged
    (64, 128, 32),   # RPL 2, last bit 31
    (100, 100, 32),  # the reference's board
    (97, 192, 8),    # RPL 3, NW 4
    (128, 256, 8),   # RPL 4, NW 4, the register-heaviest
]
NAMED_RULES = ["B3/S23", "B36/S23", "B2/S", "B3678/S34678", "B3/S012345678", "B1357/S1357", "B0/S", "B01/S8", "B/S",
               "B012345678/S012345678"]
RANDOM_RULES = [(int(b), int(s)) for b, s in np.random.default_rng(2024).integers(0, 512, (8, 2))]
RULES = NAMED_RULES + RANDOM_RULES


def _rule_id(rule):
    return rule.replace("/", "_") if isinstance(rule, str) else "b%03x_s%03x" % rule


def masks(rule):
    """(birth, survive) of "B<digits>/S<digits>" or of a pair: the test's own reading, not the library's."""
    if not isinstance(rule, str):
        return rule
    m = re.fullmatch(r"B([0-8]*)/S([0-8]*)", rule)
    return sum(1 << int(d) for d in m.group(1)), sum(1 << int(d) for d in m.group(2))


def ref_step(cells, rule, boundary, generations=1):
    """`generations` synchronous generations of an (n, H, W) uint8 array of 0 / 1 under `rule`."""
    birth, survive = masks(rule)
    bt = np.array([birth >> n & 1 for n in range(9)], np.uint8)
    st = np.array([survive >> n & 1 for n in range(9)], np.uint8)
    cur = np.ascontiguousarray(cells, dtype=np.uint8)
    h, w = cur.shape[1:]
    for _ in range(generations):
        n = np.zeros(cur.shape, np.uint8)
        if boundary == TORUS:
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dy or dx:
                        n += np.roll(cur, (dy, dx), (1, 2))
        else:
            p = np.pad(cur, ((0, 0), (1, 1), (1, 1)))
            for dy in (0, 1, 2):
                for dx in (0, 1, 2):
                    if dy != 1 or dx != 1:
                        n += p[:, dy:dy + h, dx:dx + w]
        cur = np.where(cur != 0, st[n], bt[n])
    return cur


def ref_census(cells, rule, boundary, G):
    """[(transient, period, population of B_transient)] by the definition, UNRESOLVED where t* > G."""
    n = len(cells)
    seen = [{cells[i].tobytes(): 0} for i in range(n)]
    pops = [[int(cells[i].sum())] for i in range(n)]
    out = [UNRESOLVED] * n
    open_ = set(range(n))
    cur = cells
    for t in range(1, G + 1):
        if not open_:
            break
        cur = ref_step(cur, rule, boundary)
        for i in sorted(open_):
            key = cur[i].tobytes()
            if key in seen[i]:
                mu = seen[i][key]
                out[i] = (mu, t - mu, pops[i][mu])
                open_.discard(i)
            else:
                seen[i][key] = t
                pops[i].append(int(cur[i].sum()))
    return out


def _rand(n, h, w, seed, p=0.4):  # the generator of test_gpu_batch.py
    return (np.random.default_rng(seed).random((n, h, w)) < p).astype(np.uint8)


_cache = {}


def _cached(key, make):
    """A reference computed once, shared by the tests that need it and never written to."""
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def _soup(w, h, n):
    return _cached(("soup", w, h, n), lambda: _rand(n, h, w, 1000 * w + h))


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


def _force_table(b, force=1):
    from gameoflifewithactors_amd import _lib

    _lib.check(_lib.load().gol_debug_batch_rule_table(b._h, force), "gol_debug_batch_rule_table")
    return b


def _got(result):
    return [tuple(int(a[i]) for a in result[:3]) for i in range(len(result[0]))]


# ------------------------------------------------------------------ 1. the table family against the Conway kernels
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("w,h,n", GEOMETRIES)
def test_forced_table_path_equals_the_conway_kernels(gol, w, h, n, boundary):
    b0 = _soup(w, h, n)
    with gol.BoardBatch(w, h, n, boundary) as a, gol.BoardBatch(w, h, n, boundary) as t:
        _force_table(t)
        assert a.rule == t.rule == "B3/S23"
        a.set_cells(b0)
        t.set_cells(b0)
        assert np.array_equal(t.step(1).get_cells(), a.step(1).get_cells())
        assert np.array_equal(t.step_trace(36, 6), a.step_trace(36, 6))
        cells = a.get_cells()
        assert np.array_equal(t.get_cells(), cells)
        assert a.generation == t.generation == 37
        assert np.array_equal(cells, _cached(("cells37", w, h, n, "B3/S23", boundary),
                                             lambda: ref_step(b0, "B3/S23", boundary, 37)))
        if (w, h) in ((33, 12), (100, 100)):
            a.set_cells(b0)
            t.set_cells(b0)
            ra, rt = a.cycles(600, with_steps=True), t.cycles(600, with_steps=True)
            for x, y in zip(ra[:3], rt[:3]):
                assert np.array_equal(x, y)
            assert np.array_equal(ra[3], rt[3])  # the same search on the same sequence takes the same steps
            assert (ra[3] <= 6 * 600).all()
        # the knob goes back: force = 0 is the default path again, anything but 0 / 1 is refused
        _force_table(t, 0)
        with pytest.raises(ValueError):
            _force_table(t, 2)
        assert np.array_equal(t.set_cells(cells).step(3).get_cells(), a.set_cells(cells).step(3).get_cells())


# ------------------------------------------------------------------ 2. the rule sweep
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("rule", RULES, ids=_rule_id)
@pytest.mark.parametrize("w,h,n", GEOMETRIES)
def test_rule_sweep(gol, w, h, n, rule, boundary):
    b0 = _soup(w, h, n)
    want1 = _cached(("cells1", w, h, n, rule, boundary), lambda: ref_step(b0, rule, boundary, 1))
    want37 = _cached(("cells37", w, h, n, rule, boundary), lambda: ref_step(want1, rule, boundary, 36))
    with gol.BoardBatch(w, h, n, boundary) as b:
        b.set_rule(rule).set_cells(b0)
        got1 = b.step(1).get_cells()
        assert np.array_equal(got1, want1), np.argwhere(got1 != want1)[:5]
        assert np.array_equal(b.populations(), want1.sum((1, 2)))
        got37 = b.step(36).get_cells()
        assert np.array_equal(got37, want37), np.argwhere(got37 != want37)[:5]
        assert np.array_equal(b.populations(), want37.sum((1, 2)))  # read from the packed words: a pad bit would count
    with gol.BoardBatch(w, h, n, boundary, rule=rule) as b:  # the constructor's argument, and 37 in one launch
        assert np.array_equal(b.set_cells(b0).step(37).get_cells(), want37)


@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("w,h,n", GEOMETRIES)
def test_no_pad_bit_and_no_outside_cell_ever_lives(gol, w, h, n, boundary):
    """Rules that give birth on 0: bits at or beyond W, lanes at or beyond H / RPL and the rows outside a bounded board
    would all come alive if anything read them as cells.  Populations are counted from the packed words."""
    b0 = _soup(w, h, n)
    with gol.BoardBatch(w, h, n, boundary) as b:
        b.set_rule("B012345678/S012345678").set_cells(b0).step(1)
        assert (b.populations() == w * h).all() and (b.get_cells() == 1).all()
        assert (b.step_trace(3, 1) == w * h).all()
        b.set_rule("B/S").step(1)
        assert (b.populations() == 0).all() and (b.get_cells() == 0).all()
        b.set_rule("B0/S").clear()
        trace = b.step_trace(6, 1)
        assert trace.shape == (6, n) and (trace[0::2] == w * h).all() and (trace[1::2] == 0).all(), trace[:, 0]
        assert (b.populations() == 0).all()
        assert (b.step(1).populations() == w * h).all() and (b.get_cells() == 1).all()
        assert (b.step(1).populations() == 0).all()


# ------------------------------------------------------------------ 3. the trace under a rule
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("rule", ["B3678/S34678", "B01/S8"], ids=_rule_id)
@pytest.mark.parametrize("w,h", [(33, 12), (100, 100)])
def test_trace_under_a_rule(gol, w, h, rule, boundary):
    b0 = _soup(w, h, 32)

    def curves():
        cur, rows = b0, []
        for _ in range(8):
            cur = ref_step(cur, rule, boundary, 5)
            rows.append(cur.sum((1, 2)))
        return np.array(rows, np.uint32)

    want = _cached(("trace", w, h, rule, boundary), curves)
    with gol.BoardBatch(w, h, 32, boundary, rule=rule) as b:
        got = b.set_cells(b0).step_trace(40, 5)
        assert got.shape == (8, 32) and got.dtype == np.uint32
        assert np.array_equal(got, want)
        assert b.generation == 40 and np.array_equal(b.populations(), want[-1])


# ------------------------------------------------------------------ 4. the census under a rule
CENSUS_G = 600
CENSUS_SIZES = [(33, 12), (40, 12), (16, 16)]
CENSUS_RULES = ["B36/S23", "B2/S", "B1357/S1357", "B0/S", "B01/S8"]


def _census_soup(w, h):
    return _cached(("census soup", w, h), lambda: _rand(32, h, w, 7))


def _census(w, h, rule, boundary, G=CENSUS_G):
    return _cached(("census", w, h, rule, boundary, G), lambda: ref_census(_census_soup(w, h), rule, boundary, G))


@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("rule", CENSUS_RULES, ids=_rule_id)
@pytest.mark.parametrize("w,h", CENSUS_SIZES)
def test_census_under_a_rule(gol, w, h, rule, boundary):
    """Every (transient, period, population) against the reference, unresolved boards included -- and the reference's
    own outcomes, computed for these soups apart from it, so that the comparison cannot pass by resolving nothing."""
    G = CENSUS_G
    want = _census(w, h, rule, boundary)
    resolved = [x for x in want if x != UNRESOLVED]
    periods = [lam for _, lam, _ in resolved]
    if rule == "B36/S23" and (w, h, boundary) == (33, 12, TORUS):
        assert len(resolved) == 32 and max(mu + lam for mu, lam, _ in resolved) == 600, want
    if rule == "B2/S":
        assert not resolved, want
    if rule == "B1357/S1357":
        if (w, h, boundary) == (33, 12, TORUS):
            assert periods == [124] * 32, want
        if (w, h, boundary) == (40, 12, TORUS):
            assert periods == [24] * 32, want
        if (w, h, boundary) == (16, 16, BOUNDED):
            assert periods == [30] * 32, want
        if (w, h, boundary) == (33, 12, BOUNDED):
            assert not resolved, want
    if rule == "B0/S":
        assert periods == [2] * 32, want
    if rule == "B01/S8":
        assert len(resolved) == 32, want
    with gol.BoardBatch(w, h, 32, boundary, rule=rule) as b:
        b.set_cells(_census_soup(w, h))
        res = b.cycles(G, with_steps=True)
        steps = [int(s) for s in res[3]]
        print(w, h, rule, boundary, _got(res)[:4], max(steps))
        assert _got(res) == want
        assert all(0 < s <= 6 * G for s in steps), steps
        if rule == "B36/S23" and (w, h, boundary) == (33, 12, TORUS):
            # the slowest board lies exactly on the cap: one generation less leaves it unresolved
            want599 = _census(w, h, rule, boundary, 599)
            assert UNRESOLVED in want599
            assert _got(b.cycles(599)) == want599


def _board(w, h, points):
    b = np.zeros((1, h, w), np.uint8)
    for y, x in points:
        b[0, y, x] = 1
    return b


R_PENTOMINO = [(6, 21), (6, 22), (7, 20), (7, 21), (8, 21)]
GLIDER = [(3, 2), (4, 3), (5, 1), (5, 2), (5, 3)]
# computed apart from this file's reference; cells as (y, x)
PINS = [
    (33, 12, TORUS, "B0/S", [], (0, 2, 0)),
    (33, 12, BOUNDED, "B0/S", [], (0, 2, 0)),
    (40, 12, TORUS, "B3/S23", R_PENTOMINO, (196, 1, 26)),
    (40, 12, TORUS, "B36/S23", R_PENTOMINO, (9, 1, 0)),
    (33, 12, TORUS, "B36/S23", GLIDER, (0, 528, 5)),  # as the Conway pin of test_gpu_cycles.py
    (33, 12, BOUNDED, "B2/S", [(5, 5), (5, 6)], (8, 1, 0)),
    (16, 16, TORUS, "B1357/S1357", [(3, 3)], (8, 1, 0)),
]


@pytest.mark.parametrize("w,h,boundary,rule,points,value", PINS,
                         ids=["%dx%d-%d-%s-%d" % (p[0], p[1], p[2], _rule_id(p[3]), len(p[4])) for p in PINS])
def test_census_pins(gol, w, h, boundary, rule, points, value):
    b0 = _board(w, h, points)
    with gol.BoardBatch(w, h, 1, boundary, rule=rule) as b:
        got = _got(b.set_cells(b0).cycles(CENSUS_G))
    assert got == [value]
    assert ref_census(b0, rule, boundary, CENSUS_G) == [value]


# ------------------------------------------------------------------ 5. the handle
def test_handle_semantics(gol):
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    w, h, n = 33, 12, 4
    b0 = _rand(n, h, w, 5)
    with gol.BoardBatch(w, h, n, BOUNDED) as b:
        assert b.rule == "B3/S23"
        bm, sm = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.gol_ensemble_rule(b._h, ctypes.byref(bm), ctypes.byref(sm)) == 0 and (bm.value, sm.value) == (8, 12)
        assert lib.gol_ensemble_rule(b._h, None, None) == 0  # either output may be NULL
        b.set_cells(b0).step(3)
        before = (b.get_cells(), b.generation, b.populations(), b.hashes())
        assert b.set_rule("s23/b36") is b and b.rule == "B36/S23"
        after = (b.get_cells(), b.generation, b.populations(), b.hashes())
        assert all(np.array_equal(x, y) for x, y in zip(before, after)) and b.generation == 3
        # the rule is the handle's: set_cells, both seeds and clear keep it
        assert b.set_cells(b0).rule == "B36/S23" and b.generation == 0
        assert b.seed_dotnet(list(range(n))).rule == "B36/S23"
        assert b.seed_splitmix(11).rule == "B36/S23"
        seeded = b.get_cells()
        assert np.array_equal(b.step(5).get_cells(), ref_step(seeded, "B36/S23", BOUNDED, 5))
        assert b.clear().rule == "B36/S23" and b.generation == 0
        assert b.set_rule((0x1C8, 0x1D8)).rule == "B3678/S34678"  # a pair of masks
        # a mask outside 0..0x1FF is refused: the previous rule is still reported and still runs
        for birth, survive in ((0x200, 0), (0, 0x200), (-1, 0), (0, -1), (0x200, 0x200)):
            assert lib.gol_ensemble_set_rule(b._h, birth, survive) == _lib.GOL_ERR_INVALID
            assert lib.gol_last_error()
            with pytest.raises(ValueError):
                b.set_rule((birth, survive))
            assert b.rule == "B3678/S34678"
        for text in ("B9/S23", "B3/S23/3", "B33/S2", "B3S23", ""):
            with pytest.raises(ValueError):
                b.set_rule(text)
            assert b.rule == "B3678/S34678"
        assert np.array_equal(b.set_cells(b0).step(4).get_cells(), ref_step(b0, "B3678/S34678", BOUNDED, 4))
    with pytest.raises(ValueError):
        gol.BoardBatch(w, h, n, rule="B9/S")


def test_two_batches_with_different_rules_do_not_affect_each_other(gol):
    w, h, n = 40, 12, 4
    b0 = _rand(n, h, w, 9)
    with gol.BoardBatch(w, h, n, rule="B36/S23") as a, gol.BoardBatch(w, h, n, rule="B2/S") as b, \
            gol.BoardBatch(w, h, n) as c:
        for x in (a, b, c):
            x.set_cells(b0)
        for _ in range(5):
            a.step(2)
            b.step(2)
            c.step(2)
        assert np.array_equal(a.get_cells(), ref_step(b0, "B36/S23", TORUS, 10))
        assert np.array_equal(b.get_cells(), ref_step(b0, "B2/S", TORUS, 10))
        assert np.array_equal(c.get_cells(), ref_step(b0, "B3/S23", TORUS, 10))
        assert (a.rule, b.rule, c.rule) == ("B36/S23", "B2/S", "B3/S23")


def test_census_is_read_only_under_a_rule(gol):
    w, h, n = 33, 12, 8
    b0 = _rand(n, h, w, 3)
    with gol.BoardBatch(w, h, n, TORUS, rule="B3678/S34678") as b:
        b.set_cells(b0).step(2)
        before = (b.get_cells(), b.hashes(), b.populations(), b.generation, b.rule)
        first = _got(b.cycles(300))
        assert np.array_equal(b.get_cells(), before[0]) and np.array_equal(b.hashes(), before[1])
        assert np.array_equal(b.populations(), before[2]) and b.generation == before[3] == 2 and b.rule == before[4]
        assert _got(b.cycles(300)) == first == ref_census(before[0], "B3678/S34678", TORUS, 300)
