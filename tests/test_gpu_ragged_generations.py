"""GPU tests of Generations rules (B/S/C) on ragged boards: the multi-plane streaming pass on the whole-word scratch
rows and decay planes of a byte board (gol_gen_stream_ragged, csrc/gol_gen_stream.hip; the d bytes packed into bit
planes by gol_pack_ragged_decay, csrc/gol_formats.hip), bit-exact against the numpy reference of
tests/generations_reference.py."""
import numpy as np
import pytest

import generations_reference as gref
import rule_reference as ref
from test_gpu_board_rules import GENS, RULES  # the life-like sweep's rules and call lengths, every one per case

pytestmark = pytest.mark.gpu

BYTES, GEN_RAGGED = 8, 14  # gol::Pass (csrc/gol_board.h), the value of the debug option "last_pass"
NSTATES = (3, 4, 8)  # one, two and three decay planes
ALL, BLINK = "B012345678/S012345678", "B012345678/S"
FORCE = {"rule_ragged": 2}
# the life-like sweep's shapes the Generations pass is asked on; its deepest kernel is 4 deep, so the forced depth is
# 2 ("rule_k" 8 is refused on a Generations board)
SHAPES = [(65, 5, FORCE), (1985, 9, FORCE), (1001, 40, FORCE), (8209, 40, FORCE),
          (1001, 40, {**FORCE, "rule_seg_rows": 5}), (1001, 40, {**FORCE, "rule_seg_rows": 1}),
          (65, 5, {**FORCE, "rule_k": 2}), (1985, 9, {**FORCE, "rule_k": 2}), (1001, 40, {**FORCE, "rule_k": 2})]


def _id(shape):
    w, h, opts = shape
    return f"{w}x{h}" + "".join(f"-{k}{v}" for k, v in opts.items() if k != "rule_ragged")


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


def _states(w, h, nstates, seed=0):
    """Every state present, the first cells of the board one of each."""
    rng = np.random.default_rng(500 + 17 * w + h + nstates + seed)
    s = rng.integers(0, nstates, (h, w)).astype(np.uint8)
    s.reshape(-1)[:nstates] = np.arange(nstates)
    s[-1, -nstates:] = np.arange(nstates)  # ... and the last cells of the partial word
    return s


_REF = {}


def reference(w, h, rule, nstates, boundary):
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


@pytest.mark.parametrize("boundary", [0, 1])
@pytest.mark.parametrize("nstates", NSTATES)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_ragged_generations_sweep(gol, oracle, shape, nstates, boundary):
    w, h, opts = shape
    with gol.Board(w, h, boundary, options=opts, rule=f"B3/S23/{nstates}") as b:
        for rule in RULES:
            want = reference(w, h, rule, nstates, boundary)
            assert set(np.unique(want[0])) == set(range(nstates))
            b.set_rule(f"{rule}/{nstates}")
            for g in GENS:
                b.set_states(want[0]).step(g)
                assert b.get_option("last_pass") == GEN_RAGGED
                got = b.get_states()
                assert np.array_equal(got, want[g]), f"{rule}/C{nstates} {g} generations: {int((got != want[g]).sum())} cells"
                assert b.generation == g
            b.set_states(want[0]).step(29)
            assert b.hash() == gref.gen_hash(want[29], nstates, oracle)  # the stacked hash out of the scratch planes
            b.set_states(want[0]).step(29)
            assert np.array_equal(b.get_cells(), (want[29] == 1).astype(np.uint8))


@pytest.mark.parametrize("boundary", [0, 1])
@pytest.mark.parametrize("shape", SHAPES[:4], ids=_id)
def test_no_outside_cell_ever_lives_and_no_dying_bit_leaks(gol, shape, boundary):
    w, h, opts = shape
    n = NSTATES[(SHAPES.index(shape) + boundary) % 3]
    with gol.Board(w, h, boundary, options=opts, rule=f"{ALL}/C{n}") as b:
        for g in (1, 9):
            b.clear().step(g)
            assert b.get_option("last_pass") == GEN_RAGGED
            assert popcount_words(b.save_packed()) == w * h, g
            assert int(b.get_cells().sum()) == w * h and b.population() == w * h, g
            assert np.array_equal(b.get_states(), np.ones((h, w), dtype=np.uint8)), g
        b.set_rule(f"{BLINK}/C{n}").clear()
        for g in range(1, 2 * n + 2):
            b.step(1)
            s = b.get_states()
            assert s.min() == s.max() == g % n, (g, int(s.min()), int(s.max()))
            want = w * h if g % n == 1 else 0
            assert b.population() == want and popcount_words(b.save_packed()) == want, g


def test_default_thresholds(gol):
    """A Generations board takes the pass from 2^22 cells (the byte step measured faster at 1001^2), on
    calls of at least 4 generations; the board equals the one the byte step computes."""
    with gol.Board(2049, 2049, rule="B2/S345/4") as b, gol.Board(2049, 2049, rule="B2/S345/4", options={"rule_ragged": 0}) as old:
        passes = []
        b.seed_splitmix(2)
        for g in (32, 3, 32):
            b.step(g)
            passes.append(b.get_option("last_pass"))
        assert passes == [GEN_RAGGED, BYTES, GEN_RAGGED] and b.generation == 67
        old.seed_splitmix(2).step(67)
        assert old.get_option("last_pass") == BYTES
        assert b.hash() == old.hash() and b.population() == old.population() > 0
    for w, h in ((1001, 300), (129, 127)):
        with gol.Board(w, h, rule="B2/S345/4") as b:
            b.seed_splitmix(1).step(32)
            assert b.get_option("last_pass") == BYTES


def test_mixed_calls_and_setters(gol):
    w, h, n = 1001, 300, 4
    start = _states(w, h, n)
    step = lambda s, g: gref.gen_step(s, 0x004, 0x038, n, 0, g)
    with gol.Board(w, h, rule="B2/S345/4", options=FORCE) as b:
        passes = []
        b.set_states(start)
        for g in (32, 3, 32):
            b.step(g)
            passes.append(b.get_option("last_pass"))
        assert passes == [GEN_RAGGED] * 3 and b.generation == 67
        b.set_option("rule_ragged", 0).step(3).set_option("rule_ragged", 2).step(5)  # the byte step between two passes
        assert np.array_equal(b.get_states(), step(start, 75))
        b.set_states(start).step(67)
        assert np.array_equal(b.get_states(), step(start, 67))
        # setters drop the scratch state, the decay planes with it
        b.step(32).set_states(start).step(8)
        assert np.array_equal(b.get_states(), step(start, 8))
        b.step(32).set_cells((start == 1).astype(np.uint8)).step(8)  # set_cells: every dying cell dead
        assert np.array_equal(b.get_states(), step((start == 1).astype(np.uint8), 8))
        b.step(32).clear().step(8)
        assert int(b.get_states().max()) == 0
        # another state count: the bytes are brought up to date first, then every dying cell becomes dead
        b.set_states(start).step(32)
        held = step(start, 32)
        assert b.set_rule("B2/S345/8").nstates == 8
        assert np.array_equal(b.get_states(), (held == 1).astype(np.uint8))
        assert b.step_timed(32) > 0 and b.get_option("last_pass") == GEN_RAGGED
        assert np.array_equal(b.get_states(), gref.gen_step((held == 1).astype(np.uint8), 0x004, 0x038, 8, 0, 32))
