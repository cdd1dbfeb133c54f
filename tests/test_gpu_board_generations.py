"""GPU tests of Generations rules on the single board (gol_set_generations_rule, gol_set_states / gol_get_states; DESIGN.md
4.15): the multi-plane streaming pass (csrc/gol_gen_stream.hip) on packed boards and the byte step on the (alive, d) pair
on byte boards, bit-exact against the numpy reference of tests/generations_reference.py (pinned to
tests/rule_reference.py at two states by tests/test_generations_host.py), the invariants of the planes, the handle's
semantics and the batch's Generations kernels as a second witness."""
import ctypes

import numpy as np
import pytest

import generations_reference as gref
import rule_reference as ref

pytestmark = pytest.mark.gpu

TORUS, BOUNDED = 0, 1
BYTES, GEN_STREAM = 8, 12  # gol::Pass (csrc/gol_board.h), the value of the debug option "last_pass"
NSTATES = (3, 4, 5, 8)  # every plane count, both sides of each plane boundary
RULES = ("B2/S", "B2/S345", "B34/S12", "B3/S23", "B0123/S8")
GENS = (1, 3, 7, 9, 29)  # every depth of the pass (4, 2, 1) and the remainder chains
ALL, BLINK = "B012345678/S012345678", "B012345678/S"

# (width, height, ilv (0 = the library's), options)
STREAM_SHAPES = [
    (32, 3, 1, {}),      # one block, fewer rows than K: the rows wrap several times
    (64, 5, 1, {}),
    (64, 5, 2, {}),
    (128, 7, 4, {}),     # one block of four words
    (1984, 9, 1, {}),    # exactly 62 blocks: one full strip
    (2016, 9, 1, {}),    # 63 blocks: a second strip of one block
    (4096, 40, 2, {}),   # 64 blocks, two strips
    (8192, 33, 4, {}),   # 64 blocks of four words
    (256, 40, 1, {"rule_seg_rows": 5}),  # eight segments
    (256, 40, 1, {"rule_seg_rows": 1}),  # a segment shorter than any halo
    (256, 256, 0, {}),   # the defaults of gol_create at the sizes the lanes and cooperative passes own at two states
    (2048, 64, 0, {}),
    (4096, 64, 0, {}),
]
BYTES_SHAPES = [(3, 3, 0, {}), (100, 100, 0, {}), (129, 127, 0, {}), (333, 7, 0, {})]
SHAPES = STREAM_SHAPES + BYTES_SHAPES


def _id(shape):
    w, h, ilv, opts = shape
    return f"{w}x{h}" + (f"-ilv{ilv}" if ilv else "") + "".join(f"-{k}{v}" for k, v in opts.items())


def _pass(shape):
    return GEN_STREAM if shape[0] % 32 == 0 else BYTES


def _combos(shape, boundary):
    """Two (nstates, rule) pairs per (shape, boundary), rotated so that every rule meets every state count."""
    si = SHAPES.index(shape)
    out = []
    for j in range(2):
        ni = (si + 2 * boundary + j) % 4
        out.append((NSTATES[ni], RULES[(si // 4 + ni + 2 * j + boundary) % 5]))
    return out


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


def _states(w, h, nstates, seed=0):
    """Every state present (where the board has the cells for it): tests/test_gpu_generations.py's start boards."""
    rng = np.random.default_rng(400 + 17 * w + h + nstates + seed)
    s = rng.integers(0, nstates, (h, w)).astype(np.uint8)
    flat = s.reshape(-1)
    for k in range(min(nstates, flat.size)):
        flat[k] = k
    return s


_REF = {}


def reference(w, h, rule, nstates, boundary):
    """{generations: states} of the start board of this size under the rule, computed once and never written to."""
    key = (w, h, rule, nstates, boundary)
    if key not in _REF:
        birth, survive = ref.masks(rule)
        s = _states(w, h, nstates)
        out, done = {0: s}, 0
        for g in sorted(GENS):
            s = gref.gen_step(s, birth, survive, nstates, boundary, g - done)
            out[g], done = s, g
        for v in out.values():
            v.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def popcount_words(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def test_every_rule_meets_every_state_count():
    pairs = {c for shape in SHAPES for bd in (0, 1) for c in _combos(shape, bd)}
    assert pairs == {(n, r) for n in NSTATES for r in RULES}


# ---------------------------------------------------------------- 1. the sweep
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_sweep(gol, oracle, shape, boundary):
    w, h, ilv, opts = shape
    for ci, (nstates, rule) in enumerate(_combos(shape, boundary)):
        want = reference(w, h, rule, nstates, boundary)
        with gol.Board(w, h, boundary, ilv=ilv, options=opts, rule=f"{rule}/{nstates}") as b:
            assert b.nstates == nstates and b.rule == f"{rule}/C{nstates}"
            for g in GENS:
                b.set_states(want[0]).step(g)
                got = b.get_states()
                assert np.array_equal(got, want[g]), f"{rule}/C{nstates} {g} generations: {int((got != want[g]).sum())} cells"
                assert np.array_equal(b.get_cells(), (want[g] == 1).astype(np.uint8))
                assert b.population() == int((want[g] == 1).sum())
                assert b.hash() == gref.gen_hash(want[g], nstates, oracle)
                assert b.generation == g
                assert b.get_option("last_pass") == _pass(shape)
            if ci == 0 and _pass(shape) == GEN_STREAM:  # once per packed shape: the forced depths give the same boards
                for k in (2, 1):
                    b.set_option("rule_k", k).set_states(want[0]).step(9)
                    assert np.array_equal(b.get_states(), want[9]), k
                    assert b.get_option("last_pass") == GEN_STREAM


# ---------------------------------------------------------------- 2. split calls
@pytest.mark.parametrize("nstates", NSTATES)
@pytest.mark.parametrize("shape", [(256, 40, 1, {}), (128, 7, 4, {}), (129, 127, 0, {})], ids=_id)
def test_split_calls_keep_the_decay(gol, shape, nstates):
    w, h, ilv, opts = shape
    want = reference(w, h, "B2/S345", nstates, TORUS)
    with gol.Board(w, h, TORUS, ilv=ilv, rule=f"B2/S345/{nstates}") as b:
        b.set_states(want[0]).step(4).step(0).step(5)
        assert b.generation == 9 and np.array_equal(b.get_states(), want[9])


# ---------------------------------------------------------------- 3. no outside cell ever lives, no dying bit leaks
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_no_outside_cell_ever_lives_and_no_dying_bit_leaks(gol, shape, boundary):
    w, h, ilv, opts = shape
    n = NSTATES[(SHAPES.index(shape) + boundary) % 4]
    with gol.Board(w, h, boundary, ilv=ilv, options=opts, rule=f"{ALL}/C{n}") as b:
        for g in (1, 9):
            b.clear().step(g)
            assert popcount_words(b.save_packed()) == w * h, g
            assert int(b.get_cells().sum()) == w * h and b.population() == w * h, g
            assert np.array_equal(b.get_states(), np.ones((h, w), dtype=np.uint8)), g
        b.set_rule(f"{BLINK}/C{n}").clear()
        assert b.nstates == n
        for g in range(1, 2 * n + 2):
            b.step(1)
            s = b.get_states()
            assert s.min() == s.max() == g % n, (g, int(s.min()), int(s.max()))
            want = w * h if g % n == 1 else 0
            assert b.population() == want and popcount_words(b.save_packed()) == want, g


# ---------------------------------------------------------------- 4. handle semantics
@pytest.mark.parametrize("shape", [(256, 40, 1, {}), (128, 7, 4, {}), (129, 127, 0, {})], ids=_id)
def test_setters_of_cells_leave_states_zero_and_one(gol, shape):
    w, h, ilv, _ = shape
    nstates = 8
    start = _states(w, h, nstates)
    cells = ref.soup(w, h, 5)
    with gol.Board(w, h, TORUS, ilv=ilv, rule="B2/S/8") as b:
        setters = (lambda: b.set_cells(cells), lambda: b.load_packed(b.save_packed()), lambda: b.seed_splitmix(11),
                   lambda: b.seed_dotnet(3), lambda: b.clear())
        for i, setter in enumerate(setters):
            b.set_states(start).step(1)
            before = b.get_states()
            assert before.max() == nstates - 1 and b.generation == 1
            setter()
            after = b.get_states()
            assert after.max() <= 1 and np.array_equal(after, b.get_cells()) and b.generation == 0, i
            if i == 1:  # load_packed of the board's own snapshot: the alive cells, and nothing else
                assert np.array_equal(after, (before == 1).astype(np.uint8))
            # and the decay is gone from both buffers: a generation later no cell is past state 2
            assert b.step(1).get_states().max() <= 2, i
        assert np.array_equal(b.set_cells(cells).get_states(), cells)


@pytest.mark.parametrize("shape", [(64, 5, 2, {}), (129, 127, 0, {})], ids=_id)
def test_place_rle_onto_a_dying_cell_makes_it_alive(gol, shape):
    w, h, ilv, _ = shape
    s = np.full((h, w), 3, dtype=np.uint8)
    s[0, 0] = 2
    with gol.Board(w, h, BOUNDED, ilv=ilv, rule="B/S/5") as b:
        b.set_states(s).place_rle("bo$2bo$3o!", 1, 1)
        want = s.copy()
        for x, y in ((1, 0), (2, 1), (0, 2), (1, 2), (2, 2)):
            want[1 + y, 1 + x] = 1
        assert np.array_equal(b.get_states(), want)
        assert np.array_equal(b.step(1).get_states(), gref.gen_step(want, 0, 0, 5, BOUNDED, 1))


@pytest.mark.parametrize("shape", [(256, 40, 1, {}), (129, 127, 0, {})], ids=_id)
def test_rule_changes_keep_or_clear_the_dying_cells(gol, shape):
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    w, h, ilv, _ = shape
    start = _states(w, h, 4)
    with gol.Board(w, h, TORUS, ilv=ilv, rule="B2/S345/4") as b, gol.Board(w, h, TORUS, ilv=ilv, rule="B2/S345") as fresh:
        b.set_states(start).step(3)
        held = b.get_states()
        assert held.max() == 3
        assert b.set_rule("B34/S12").rule == "B34/S12/C4" and b.nstates == 4  # set_rule keeps nstates and dying cells
        assert np.array_equal(b.get_states(), held) and b.generation == 3
        bi, su, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.gol_rule(b._h, ctypes.byref(bi), ctypes.byref(su)) == 0 and (bi.value, su.value) == (0x018, 0x006)
        assert lib.gol_generations_rule(b._h, ctypes.byref(bi), ctypes.byref(su), ctypes.byref(n)) == 0
        assert (bi.value, su.value, n.value) == (0x018, 0x006, 4)
        assert b.set_rule("B2/S345/4").rule == "B2/S345/C4"  # the same nstates: dying cells stay
        assert np.array_equal(b.get_states(), held) and b.generation == 3
        assert np.array_equal(b.step(2).get_states(), gref.gen_step(held, 0x004, 0x038, 4, TORUS, 2))
        held = b.get_states()
        alive = (held == 1).astype(np.uint8)
        assert b.set_rule("B2/S345/5").nstates == 5  # another nstates: every dying cell dead, the rest untouched
        assert np.array_equal(b.get_states(), alive) and b.generation == 5
        assert np.array_equal(b.step(6).get_states(), gref.gen_step(alive, 0x004, 0x038, 5, TORUS, 6))
        b.set_states(start % 4).set_rule((0x004, 0x038, 4))
        b.set_states(start).step(1)
        held = b.get_states()
        assert b.set_rule((0x004, 0x038, 2)).rule == "B2/S345" and b.nstates == 2  # two states after four
        assert np.array_equal(b.get_states(), (held == 1).astype(np.uint8)) and b.generation == 1
        for gens in (1, 40):  # ... runs the two-state passes: what a fresh board of the shape reports under the rule
            cells = ref.soup(w, h, 6)
            fresh.set_cells(cells).step(gens)
            b.set_cells(cells).step(gens)
            assert b.get_option("last_pass") == fresh.get_option("last_pass") not in (GEN_STREAM,)
            assert np.array_equal(b.get_cells(), fresh.get_cells())
            assert np.array_equal(b.get_cells(), ref.ref_step(cells, 0x004, 0x038, TORUS, gens))
            assert b.hash() == fresh.hash()


def test_invalid_arguments_leave_the_board_unchanged(gol):
    from gameoflifewithactors_amd import _lib

    lib = _lib.load()
    w, h, nstates = 64, 5, 4
    start = _states(w, h, nstates)
    with gol.Board(w, h, TORUS, ilv=2, rule="B2/S345/4") as b:
        b.set_states(start).step(2)
        held, hashed = b.get_states(), b.hash()
        bad = start.copy()
        bad[h - 1, w - 1] = nstates
        ptr = bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        assert lib.gol_set_states(b._h, ptr, bad.size) == _lib.GOL_ERR_INVALID
        with pytest.raises(ValueError):
            b.set_states(bad)
        good = np.ascontiguousarray(start)
        ptr = good.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        for length in (good.size - 1, good.size + 1, 0):
            assert lib.gol_set_states(b._h, ptr, length) == _lib.GOL_ERR_INVALID
            assert lib.gol_get_states(b._h, ptr, length) == _lib.GOL_ERR_INVALID
        assert lib.gol_set_states(b._h, None, good.size) == _lib.GOL_ERR_INVALID
        for n in (1, 9, 0, -1):
            assert lib.gol_set_generations_rule(b._h, 4, 0, n) == _lib.GOL_ERR_INVALID, n
        for masks in ((0x200, 0), (0, 0x200), (-1, 0)):
            assert lib.gol_set_generations_rule(b._h, *masks, 3) == _lib.GOL_ERR_INVALID, masks
        with pytest.raises(ValueError):
            b.set_rule("B2/S/9")
        with pytest.raises(ValueError):
            b.set_option("rule_k", 8)
        bi, su, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.gol_generations_rule(b._h, None, ctypes.byref(su), ctypes.byref(n)) == _lib.GOL_ERR_INVALID
        assert lib.gol_generations_rule(b._h, ctypes.byref(bi), ctypes.byref(su), None) == _lib.GOL_ERR_INVALID
        assert b.rule == "B2/S345/C4" and b.generation == 2 and b.hash() == hashed
        assert np.array_equal(b.get_states(), held)


def test_pass_timing_is_refused_and_step_timed_times_the_pass(gol):
    from gameoflifewithactors_amd import _lib

    with gol.Board(8192, 512, options={"coop": 0}) as b:
        b.seed_splitmix(1)
        assert len(b.pass_timing()) == 1
        b.set_rule("B3/S23/3")  # Conway's masks, three states: still no pass the timing measures
        with pytest.raises(NotImplementedError):
            b.pass_timing()
        arr = (ctypes.c_double * 1)()
        assert _lib.load().gol_pass_timing(b._h, 1, arr, arr, arr) == _lib.GOL_ERR_UNSUPPORTED
        done = b.generation
        assert b.step_timed(9) > 0 and b.get_option("last_pass") == GEN_STREAM and b.generation == done + 9


@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
def test_a_ragged_board_whose_state_is_in_scratch_rows_takes_the_rule(gol, boundary):
    cells = ref.soup(1001, 40, 8)
    with gol.Board(1001, 40, boundary) as b:
        b.set_cells(cells).step(32)
        assert b.get_option("last_pass") not in (BYTES, 1)  # a multi-generation pass: the state sits in scratch rows
        b.set_rule("B2/S345/4").step(3)
        assert b.get_option("last_pass") == BYTES
        now = ref.ref_step(cells, 8, 12, boundary, 32)
        assert np.array_equal(b.get_states(), gref.gen_step(now, 0x004, 0x038, 4, boundary, 3)) and b.generation == 35


def test_two_state_boards_take_states_zero_and_one(gol):
    cells = ref.soup(1001, 40, 9)
    with gol.Board(1001, 40) as b:
        b.set_states(cells).step(32)  # the ragged multi-generation pass, then the state bytes out of its scratch rows
        assert b.generation == 32
        assert np.array_equal(b.get_states(), ref.ref_step(cells, 8, 12, TORUS, 32))
        with pytest.raises(ValueError):
            b.set_states(cells * 2)


@pytest.mark.parametrize("shape", [(256, 40, 1, {}), (129, 127, 0, {})], ids=_id)
def test_snapshots_carry_the_alive_plane_only(gol, tmp_path, shape):
    w, h, ilv, _ = shape
    start = _states(w, h, 4)
    path = str(tmp_path / "gen.snap")
    with gol.Board(w, h, TORUS, ilv=ilv, rule="B2/S345/4") as b:
        b.set_states(start).step(3)
        now = b.get_states()
        assert now.max() == 3
        b.save(path)
        assert np.array_equal(b.get_states(), now)  # saving changes nothing
    alive = (now == 1).astype(np.uint8)
    with gol.Board.from_snapshot(path) as plain, gol.Board.from_snapshot(path, rule="B2/S345/4") as again:
        assert plain.rule == "B3/S23" and again.rule == "B2/S345/C4"
        assert np.array_equal(plain.get_cells(), alive) and np.array_equal(again.get_states(), alive)
        assert np.array_equal(again.step(5).get_states(), gref.gen_step(alive, 0x004, 0x038, 4, TORUS, 5))


# ---------------------------------------------------------------- 5. against the batch
@pytest.mark.parametrize("size", [(100, 100), (128, 256)], ids=lambda s: "%dx%d" % s)
def test_a_board_equals_a_batch_of_one(gol, size):
    w, h = size
    start = _states(w, h, 4)
    with gol.Board(w, h, TORUS, rule="B2/S345/4") as b, gol.BoardBatch(w, h, 1, TORUS, rule="B2/S345/4") as batch:
        b.set_states(start).step(29)
        batch.set_states(start[None]).step(29)
        assert np.array_equal(b.get_states(), batch.get_states()[0])
        assert b.hash() == int(batch.hashes()[0]) and b.population() == int(batch.populations()[0])


# ---------------------------------------------------------------- 6. two states unchanged
@pytest.mark.parametrize("boundary", [TORUS, BOUNDED])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_two_states_are_the_life_like_board(gol, shape, boundary):
    w, h, ilv, opts = shape
    rule = RULES[SHAPES.index(shape) % 5]
    cells = ref.soup(w, h, 1000 * w + h)
    want = ref.ref_step(cells, *ref.masks(rule), boundary, 9)
    with gol.Board(w, h, boundary, ilv=ilv, options=opts, rule=f"{rule}/2") as b:
        assert b.nstates == 2 and b.rule == rule
        b.set_states(cells).step(9)
        assert b.get_option("last_pass") != GEN_STREAM
        assert np.array_equal(b.get_states(), b.get_cells()) and np.array_equal(b.get_cells(), want)


# ---------------------------------------------------------------- 7. several GPUs
def test_multi_gpu_boards_refuse_more_than_two_states(gol):
    from gameoflifewithactors_amd import _lib

    if _lib.device_count() < 2:
        pytest.skip("needs two devices")
    with gol.Board(256, 96, num_gpus=2) as b:
        assert _lib.load().gol_set_generations_rule(b._h, 8, 12, 3) == _lib.GOL_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            b.set_rule("B3/S23/3")
        assert b.rule == "B3/S23" and b.nstates == 2
        assert b.set_rule("B3/S23/2").rule == "B3/S23"


# ---------------------------------------------------------------- the driver
def test_driver_runs_brians_brain(gol):
    from gameoflifewithactors_amd import driver

    frames = []
    agent = driver.UpdateAgent(on_frame=lambda p: frames.append(np.array(p, copy=True)))
    with driver.run(seed=42, agent=agent, emit="pixels", rule="B2/S/3") as game:
        assert game.board.rule == "B2/S/C3" and game.board.nstates == 3
        states = game.board.get_states()
        for _ in range(5):
            game.update_view()
        assert game.board.get_option("last_pass") == BYTES
    assert len(frames) == 5
    for i, frame in enumerate(frames):
        states = gref.gen_step(states, 0x004, 0, 3, TORUS, 1)
        assert np.array_equal(frame.reshape(100, 100), (states == 1) * 128), i
