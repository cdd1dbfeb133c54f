"""GPU tests of one life-like rule per board of a batch (BoardBatch.set_rules / rules over gol_ensemble_set_rules /
gol_ensemble_rules; the per-board family of csrc/gol_batch.hip and csrc/gol_cycles.hip): step,
population trace and cycle census where every wave runs its own board under its own rule.

The reference is tests/rule_reference.py (one board, one rule, numpy; pinned to the CPU oracle under B3/S23 by
tests/test_board_rules_host.py), run board by board.  37 boards are no multiple of the 4 waves of a workgroup and the
8 rules no divisor of 37, so every workgroup mixes rules and the last one is partly empty.
"""
import ctypes

import numpy as np
import pytest

import rule_reference as ref
import test_gpu_board_rules as board_rules

pytestmark = pytest.mark.gpu

TORUS, BOUNDED = 0, 1
UNRESOLVED = (-1, 0, 0)
ALL, NONE = "B012345678/S012345678", "B/S"

# (W, H, words per row, rows per lane): one geometry per NW and per RPL of the batch kernels
GEOMETRIES = [(3, 3, 1, 1), (33, 12, 2, 1), (96, 192, 3, 3), (100, 100, 4, 2), (128, 256, 4, 4)]
SIZES = [g[:2] for g in GEOMETRIES]
LIST = tuple(board_rules.RULES) + ("B3/S23",)  # the single board's seven rules and Conway's: board i runs LIST[i % 8]
N = 37
STEPS = (1, 7, 29)


def _rules(n):
    return [LIST[i % 8] for i in range(n)]


_cache = {}


def _cached(key, make):
    """A reference computed once, shared by the tests that need it and never written to."""
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def _soups(w, h, n):
    return _cached(("soups", w, h, n), lambda: np.stack([ref.soup(w, h, 7000 + 131 * w + h + i) for i in range(n)]))


def _ref_run(cells, rules, boundary, generations):
    """Every board `generations` further under its own rule."""
    return np.stack([ref.ref_step(c, *ref.masks(r), boundary, generations) for c, r in zip(cells, rules)])


def _ref_after(w, h, n, boundary, g):
    """The n soups after g generations, each under LIST[i % 8]; g walks up STEPS and the trace's samples."""
    chain = sorted(set(STEPS) | {3, 6, 9, 12})
    if g == 0:
        return _soups(w, h, n)
    prev = max([x for x in chain if x < g], default=0)
    return _cached(("after", w, h, n, boundary, g),
                   lambda: _ref_run(_ref_after(w, h, n, boundary, prev), _rules(n), boundary, g - prev))


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


def _waves(b, waves):
    from gameoflifewithactors_amd import _lib

    _lib.check(_lib.load().gol_debug_batch_group_waves(b._h, waves), "gol_debug_batch_group_waves")
    return b


def _got(result):
    return [tuple(int(a[i]) for a in result[:3]) for i in range(len(result[0]))]


def test_the_geometries_cover_every_words_per_row_and_rows_per_lane(gol):
    for w, h, nw, rpl in GEOMETRIES:
        assert gol.batch_supported(w, h) == rpl != 0 and (w + 31) // 32 == nw, (w, h)
    assert {g[2] for g in GEOMETRIES} == {1, 2, 3, 4} == {g[3] for g in GEOMETRIES}
    assert len(LIST) == 8 == len(set(LIST)) and LIST[:7] == tuple(board_rules.RULES)


# ------------------------------------------------------------------ 1. step
def _check_steps(gol, w, h, n, boundary, waves):
    with gol.BoardBatch(w, h, n, boundary) as b:
        _waves(b, waves).set_rules(_rules(n)).set_cells(_soups(w, h, n))
        done = 0
        for g in STEPS:
            got = b.step(g - done).get_cells()
            done = g
            want = _ref_after(w, h, n, boundary, g)
            wrong = sorted(set(np.argwhere(got != want)[:, 0].tolist()))
            assert not wrong, (g, wrong[:8], [_rules(n)[i] for i in wrong[:8]])
            assert b.generation == g
        assert np.array_equal(b.populations(), want.sum((1, 2)))


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("w,h", SIZES)
def test_every_board_steps_under_its_own_rule(gol, w, h, boundary, waves):
    _check_steps(gol, w, h, N, boundary, waves)


def test_more_boards_than_simds_each_under_its_own_rule(gol):
    """1100 boards on a chip of 1024 SIMDs, as test_gpu_batch.py::test_more_boards_than_simds: a slip in the index a
    wave reads the table at shows in some board."""
    _check_steps(gol, 33, 12, 1100, TORUS, 4)


# ------------------------------------------------------------------ 2. no rule leaks between waves
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("w,h", SIZES)
def test_no_rule_leaks_between_waves(gol, w, h, boundary, waves):
    """Neighbouring boards under opposite rules, from empty: a wave that read its neighbour's entry, or entry 0, or the
    rule of another wave of its workgroup, turns a W*H into a 0 or the reverse."""
    want = np.array([w * h, 0] * N, np.int64)[:N]
    for born in (ALL, "B0/S"):  # B0/S from empty: all alive after every odd generation
        with gol.BoardBatch(w, h, N, boundary) as b:
            _waves(b, waves).set_rules([born if i % 2 == 0 else NONE for i in range(N)])
            assert (b.populations() == 0).all()
            assert np.array_equal(b.step(1).populations(), want), born
            assert np.array_equal(b.step(8).populations(), want), born
            assert b.generation == 9
            assert np.array_equal(b.get_cells().sum((1, 2)), want)


# ------------------------------------------------------------------ 3. trace
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("w,h", SIZES)
def test_trace_under_the_table(gol, w, h, boundary, waves):
    want = np.array([_ref_after(w, h, N, boundary, g).sum((1, 2)) for g in (3, 6, 9, 12)], np.uint32)
    with gol.BoardBatch(w, h, N, boundary) as b:
        _waves(b, waves).set_rules(_rules(N)).set_cells(_soups(w, h, N))
        got = b.step_trace(12, every=3)
        assert got.shape == (4, N) and got.dtype == np.uint32
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        assert b.generation == 12 and np.array_equal(b.get_cells(), _ref_after(w, h, N, boundary, 12))


# ------------------------------------------------------------------ 4. census
# Soups chosen so that most boards settle: Seeds, the replicator and B0/S8 never do from a random soup on a board of
# any size, so besides two small soups (across the first word boundary) every rule also gets a single cell, an empty
# and a full board.  Group i // 8 picks the pattern, i % 8 the rule.
CENSUS_PATTERNS = (5, 3, "cell", "empty", "full")
CENSUS_G = {(3, 3): 64, (33, 12): 1500, (96, 192): 6000, (100, 100): 6000, (128, 256): 6000}


def _census_soups(w, h):
    def make():
        out = np.zeros((N, h, w), np.uint8)
        for i in range(N):
            k = CENSUS_PATTERNS[(i // 8) % len(CENSUS_PATTERNS)]
            if k == "full":
                out[i] = 1
            elif k == "cell":
                out[i, h // 2, min(w - 1, 27)] = 1
            elif k != "empty":
                ph, pw = min(h, k), min(w, k)
                y0, x0 = (h - ph) // 2, max(0, min(w - pw, 27))
                out[i, y0:y0 + ph, x0:x0 + pw] = ref.soup(pw, ph, 5000 + 100 * w + i, 0.45)
        return out

    return _cached(("census soups", w, h), make)


def _dictionary_census(cells, rule, boundary, G):
    """(transient, period, population of B_transient) of one board by the definition, UNRESOLVED where t* > G."""
    birth, survive = ref.masks(rule)
    seen, pops, cur = {cells.tobytes(): 0}, [int(cells.sum())], cells
    for t in range(1, G + 1):
        cur = ref.ref_step(cur, birth, survive, boundary, 1)
        key = cur.tobytes()
        if key in seen:
            return seen[key], t - seen[key], pops[seen[key]]
        seen[key] = t
        pops.append(int(cur.sum()))
    return UNRESOLVED


@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("w,h", SIZES)
def test_census_under_the_table(gol, w, h, boundary):
    """Board by board against the uniform path (one batch per rule under set_rule, the same cells: the code
    tests/test_gpu_rules.py pins), and at 3 x 3 and 33 x 12 against a dictionary search over the reference.  At least
    three quarters of the boards resolve in whichever the table is compared with, so that "unresolved equals
    unresolved" cannot carry the comparison; the call is read-only."""
    G = CENSUS_G[(w, h)]
    soups = _census_soups(w, h)
    rules = _rules(N)
    uniform = [None] * N
    with gol.BoardBatch(w, h, N, boundary) as u:
        for rule in LIST:
            res = _got(u.set_rule(rule).set_cells(soups).cycles(G))
            for i in range(N):
                if rules[i] == rule:
                    uniform[i] = res[i]
    resolved = [x for x in uniform if x != UNRESOLVED]
    print(w, h, boundary, "G", G, "resolved", len(resolved), "of", N, "periods", sorted({x[1] for x in resolved}))
    assert 4 * len(resolved) >= 3 * N, uniform
    assert len({x for x in resolved}) >= 6, uniform  # and not all the same answer
    with gol.BoardBatch(w, h, N, boundary) as b:
        b.set_rules(rules).set_cells(soups).step(2)
        soups2 = b.get_cells()
        before = (soups2, b.hashes(), b.populations(), b.generation, b.rules)
        b.cycles(G)
        after = (b.get_cells(), b.hashes(), b.populations(), b.generation, b.rules)
        assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3:] == after[3:]
        assert b.generation == 2
        res = b.set_cells(soups).cycles(G, with_steps=True)
        got = _got(res)
        assert got == uniform, [(i, rules[i], got[i], uniform[i]) for i in range(N) if got[i] != uniform[i]][:6]
        assert all(0 < s <= 6 * G for s in res[3])
    if (w, h) in ((3, 3), (33, 12)):
        want = _cached(("dictionary census", w, h, boundary),
                       lambda: [_dictionary_census(soups[i], rules[i], boundary, G) for i in range(N)])
        assert 4 * sum(x != UNRESOLVED for x in want) >= 3 * N, want
        assert got == want, [(i, rules[i], got[i], want[i]) for i in range(N) if got[i] != want[i]][:6]


# ------------------------------------------------------------------ 5. a uniform table is the uniform rule
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("rule", ["B3/S23", "B36/S23", "B3678/S34678"])
@pytest.mark.parametrize("w,h", SIZES)
def test_a_uniform_table_equals_the_uniform_rule(gol, w, h, rule, boundary):
    soups = _soups(w, h, N)
    with gol.BoardBatch(w, h, N, boundary) as t, gol.BoardBatch(w, h, N, boundary, rule=rule) as u:
        t.set_rules([rule] * N).set_cells(soups)
        u.set_cells(soups)
        assert t.rule == u.rule == rule and t.rules == u.rules == [rule] * N
        rt, ru = t.cycles(200, with_steps=True), u.cycles(200, with_steps=True)
        for x, y in zip(rt, ru):
            assert np.array_equal(x, y)
        assert np.array_equal(t.step(7).get_cells(), u.step(7).get_cells())
        assert np.array_equal(t.hashes(), u.hashes())
        assert np.array_equal(t.step_trace(6, 2), u.step_trace(6, 2))
        assert np.array_equal(t.get_cells(), _cached(("uniform13", w, h, rule, boundary),
                                                     lambda: _ref_run(soups, [rule] * N, boundary, 13)))


# ------------------------------------------------------------------ 6. the handle
def test_rules_round_trip(gol):
    w, h, n = 33, 12, 5
    with gol.BoardBatch(w, h, n) as b:
        assert b.rules == ["B3/S23"] * n and b.rule == "B3/S23"
        assert b.set_rules(["B36/S23", "s23/b36", " 23/36 ", (0x1C8, 0x1D8), "b/s"]) is b
        assert b.rules == ["B36/S23", "B36/S23", "B36/S23", "B3678/S34678", "B/S"]
        b.set_rules(np.array([[8, 12], [0x48, 12], [0, 0], [0x1FF, 0x1FF], [1, 256]], np.int64))
        assert b.rules == ["B3/S23", "B36/S23", "B/S", ALL, "B0/S8"]
        b.set_rules(np.array([[1, 2]] * n, np.uint16))
        assert b.rules == ["B0/S1"] * n and b.rule == "B0/S1"
        for bad in (np.zeros((n, 3), np.int64), np.zeros(n, np.int64), np.zeros((n, 2), np.float64)):
            with pytest.raises(ValueError):
                b.set_rules(bad)
        with pytest.raises(ValueError):
            b.set_rules(["B3/S23"] * (n - 1) + ["B9/S"])
        assert b.rules == ["B0/S1"] * n


def test_handle_semantics(gol):
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    w, h, n = 33, 12, N
    soups, rules = _soups(w, h, n), _rules(n)
    with gol.BoardBatch(w, h, n, BOUNDED) as b:
        b.set_cells(soups).step(3)  # under B3/S23
        before = (b.get_cells(), b.generation, b.populations(), b.hashes())
        b.set_rules(rules)
        after = (b.get_cells(), b.generation, b.populations(), b.hashes())
        assert all(np.array_equal(x, y) for x, y in zip(before, after)) and b.generation == 3  # only the future
        assert b.rules == list(rules)
        # the boards differ: the one rule is not defined, the outputs stay as they were, the message names the way out
        with pytest.raises(NotImplementedError, match="gol_ensemble_rules"):
            b.rule
        bm, sm = ctypes.c_int(-5), ctypes.c_int(-6)
        assert lib.gol_ensemble_rule(b._h, ctypes.byref(bm), ctypes.byref(sm)) == _lib.GOL_ERR_UNSUPPORTED
        assert (bm.value, sm.value) == (-5, -6)
        # gol_ensemble_rules: either output may be NULL, n is count
        bs, ss = (ctypes.c_int * n)(), (ctypes.c_int * n)()
        assert lib.gol_ensemble_rules(b._h, bs, None, n) == 0 and lib.gol_ensemble_rules(b._h, None, ss, n) == 0
        assert list(zip(bs, ss)) == [ref.masks(r) for r in rules]
        assert lib.gol_ensemble_rules(b._h, None, None, n) == 0
        assert lib.gol_ensemble_rules(b._h, bs, ss, n - 1) == _lib.GOL_ERR_INVALID
        # set_cells, both seeds and clear keep the table
        assert b.set_cells(soups).rules == list(rules) and b.generation == 0
        assert b.seed_dotnet(list(range(n))).rules == list(rules)
        assert b.seed_splitmix(11).rules == list(rules)
        seeded = b.get_cells()
        assert np.array_equal(b.step(5).get_cells(), _ref_run(seeded, rules, BOUNDED, 5))
        assert b.clear().rules == list(rules) and b.generation == 0 and (b.populations() == 0).all()

        # refusals: the table is as it was, which the step after them shows
        birth = np.array([ref.masks(r)[0] for r in reversed(rules)], np.intc)  # a table that would change every board
        survive = np.array([ref.masks(r)[1] for r in reversed(rules)], np.intc)
        bp, sp = birth.ctypes.data_as(_lib.ip), survive.ctypes.data_as(_lib.ip)
        for args in ((bp, sp, n - 1), (bp, sp, n + 1), (bp, sp, 0), (None, sp, n), (bp, None, n)):
            assert lib.gol_ensemble_set_rules(b._h, *args) == _lib.GOL_ERR_INVALID, args[2]
            assert lib.gol_last_error()
        for bad in (0x200, -1):  # at the last index: the whole table is judged before any of it is used
            for column in (birth, survive):
                keep = int(column[-1])
                column[-1] = bad
                assert lib.gol_ensemble_set_rules(b._h, bp, sp, n) == _lib.GOL_ERR_INVALID
                assert b"0x1FF" in lib.gol_last_error()
                with pytest.raises(ValueError):
                    b.set_rules(np.stack([birth, survive], 1))
                column[-1] = keep
        with pytest.raises(ValueError):
            b.set_rules(rules[:-1])
        assert b.rules == list(rules)
        assert np.array_equal(b.set_cells(soups).step(7).get_cells(), _ref_after(w, h, n, BOUNDED, 7))

        # one rule again: the batch is a uniform batch
        assert b.set_rule("B36/S23").rule == "B36/S23" and b.rules == ["B36/S23"] * n
        with gol.BoardBatch(w, h, n, BOUNDED, rule="B36/S23") as fresh:
            assert np.array_equal(b.set_cells(soups).step(9).get_cells(), fresh.set_cells(soups).step(9).get_cells())
            assert np.array_equal(b.step_trace(4, 2), fresh.step_trace(4, 2))
            assert _got(b.cycles(100)) == _got(fresh.cycles(100))
        # ... and a table again
        assert np.array_equal(b.set_rules(rules).set_cells(soups).step(1).get_cells(), _ref_after(w, h, n, BOUNDED, 1))
    # a table where all boards agree has one rule
    with gol.BoardBatch(w, h, 3) as c:
        assert c.set_rules(["B2/S"] * 3).rule == "B2/S"
        assert c.set_rules(["B2/S", "B2/S", "B2/S0"]).rules[2] == "B2/S0"
        with pytest.raises(NotImplementedError):
            c.rule


def test_two_batches_with_different_tables_do_not_affect_each_other(gol):
    w, h, n = 33, 12, N
    soups, rules = _soups(w, h, n), _rules(n)
    shifted = rules[3:] + rules[:3]
    with gol.BoardBatch(w, h, n) as a, gol.BoardBatch(w, h, n) as b, gol.BoardBatch(w, h, n) as c:
        a.set_rules(rules).set_cells(soups)
        b.set_rules(shifted).set_cells(soups)
        c.set_cells(soups)  # and one without a table
        for g in (1, 2, 4):
            a.step(g)
            b.step(g)
            c.step(g)
        assert np.array_equal(a.get_cells(), _ref_after(w, h, n, TORUS, 7))
        assert np.array_equal(b.get_cells(), _ref_run(soups, shifted, TORUS, 7))
        assert np.array_equal(c.get_cells(), _ref_run(soups, ["B3/S23"] * n, TORUS, 7))
        assert a.rules == list(rules) and b.rules == shifted and c.rule == "B3/S23"
