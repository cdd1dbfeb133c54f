"""GPU tests of life-like rules on ragged boards (width not a multiple of 32): the rule-generic streaming pass on the
whole-word scratch rows of a byte board (gol_rule_stream_ragged, csrc/gol_rule_step.hip), bit-exact
against the numpy reference of tests/rule_reference.py, the B0 invariants at the pad bits, the default thresholds, and
the state that stays in the scratch rows between calls."""
import numpy as np
import pytest

import rule_reference as ref
from test_gpu_board_rules import GENS, RULES

pytestmark = pytest.mark.gpu

BYTES, STREAM_RAGGED, RULE_RAGGED = 8, 6, 13  # gol::Pass (csrc/gol_board.h), the value of the debug option "last_pass"
ALL = "B012345678/S012345678"
FORCE = {"rule_ragged": 2}
SMALL = {"rule_ragged": 2, "wave_resident": 0}  # within the single-wave pass's 128 x 256

# (width, height, options)
SHAPES = [
    (65, 5, SMALL),     # one real cell in the last word; windows over three words; fewer rows than K
    (95, 7, SMALL),     # 31 real cells in the last word
    (100, 300, FORCE),  # the reference's width on a tall board
    (1983, 9, FORCE),   # the partial block on lane 62, the last stored lane
    (1985, 9, FORCE),   # the partial block alone in a second strip
    (2017, 9, FORCE),   # 64 words
    (1001, 40, {**FORCE, "rule_seg_rows": 5}),  # forced segment lengths
    (1001, 40, {**FORCE, "rule_seg_rows": 1}),
    (8209, 40, FORCE),  # five strips
    (65, 5, {**SMALL, "rule_k": 8}),  # the 8-deep kernels
    (1985, 9, {**FORCE, "rule_k": 8}),
    (1001, 40, {**FORCE, "rule_k": 8}),
]


def _id(shape):
    w, h, opts = shape
    return f"{w}x{h}" + "".join(f"-{k}{v}" for k, v in opts.items() if k not in ("rule_ragged", "wave_resident"))


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


_REF = {}


def reference(w, h, rule, boundary):
    """{generations: cells} of the 40 % soup of this size under the rule, computed once and never written to."""
    key = (w, h, rule, boundary)
    if key not in _REF:
        birth, survive = ref.masks(rule)
        cells = ref.soup(w, h, 1000 * w + h)
        out, done = {0: cells}, 0
        for g in sorted(GENS):
            cells = ref.ref_step(cells, birth, survive, boundary, g - done)
            out[g], done = cells, g
        for v in out.values():
            v.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def popcount_words(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


# ---------------------------------------------------------------- the sweep
@pytest.mark.parametrize("boundary", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_ragged_rule_sweep(gol, shape, boundary):
    """Whole boards, bit-exact, every call on the ragged rule pass."""
    w, h, opts = shape
    with gol.Board(w, h, boundary, options=opts) as b:
        assert b.get_option("rule_ragged") == 2
        for rule in RULES:
            b.set_rule(rule)
            want = reference(w, h, rule, boundary)
            for g in GENS:
                b.set_cells(want[0]).step(g)
                assert b.get_option("last_pass") == RULE_RAGGED
                got = b.get_cells()
                assert np.array_equal(got, want[g]), f"{rule} {g} generations: {int((got != want[g]).sum())} cells differ"
                assert b.generation == g


# ---------------------------------------------------------------- no outside cell ever lives
@pytest.mark.parametrize("boundary", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_no_outside_cell_ever_lives(gol, shape, boundary):
    """An empty board under B012345678/S012345678 holds exactly W H cells after 1 and 9 generations, counted from the
    cells and from the snapshot words; under B0/S it alternates W H, 0.  A pad bit of the partial word that is ever
    stored, unpacked or counted breaks it."""
    w, h, opts = shape
    with gol.Board(w, h, boundary, options=opts, rule=ALL) as b:
        for g in (1, 9):
            b.clear().step(g)
            assert b.get_option("last_pass") == RULE_RAGGED
            assert popcount_words(b.save_packed()) == w * h, g
            assert int(b.get_cells().sum()) == w * h and b.population() == w * h, g
        b.set_rule("B0/S").clear()
        for g in range(1, 10):
            b.step(1)
            want = w * h if g % 2 else 0
            assert b.population() == want and popcount_words(b.save_packed()) == want, g
        assert b.get_option("last_pass") == RULE_RAGGED


# ---------------------------------------------------------------- the default thresholds
def test_default_thresholds(gol):
    cells = ref.soup(1001, 300, 11)
    with gol.Board(1001, 300, rule="B36/S23") as b:
        assert b.get_option("rule_ragged") == 1
        b.set_cells(cells).step(32)
        assert b.get_option("last_pass") == RULE_RAGGED
        b.step(3)
        assert b.get_option("last_pass") == BYTES
        assert np.array_equal(b.get_cells(), ref.ref_step(cells, 0x048, 0x00C, 0, 35))
        b.set_option("rule_ragged", 0).step(32)
        assert b.get_option("last_pass") == BYTES
        with pytest.raises(ValueError):
            b.set_option("rule_ragged", 3)
    with gol.Board(129, 127, rule="B36/S23") as b:
        b.seed_splitmix(1).step(32)
        assert b.get_option("last_pass") == BYTES
    with gol.Board(63, 600, rule="B36/S23", options=FORCE) as b:  # narrower than 64 cells: the byte step
        b.seed_splitmix(1).step(32)
        assert b.get_option("last_pass") == BYTES


# ---------------------------------------------------------------- the state in the scratch rows
@pytest.mark.parametrize("boundary", [0, 1])
def test_observables_out_of_the_scratch_rows(gol, boundary):
    w, h = 1001, 300
    cells = ref.soup(w, h, 12)
    want = ref.ref_step(cells, 0x048, 0x00C, boundary, 32)
    with gol.Board(w, h, boundary, rule="B36/S23") as b, gol.Board(w, h, boundary) as fresh:
        fresh.set_cells(want)

        def again():  # every observable read straight after a pass: the state sits in the scratch rows
            b.set_cells(cells).step(32)
            assert b.get_option("last_pass") == RULE_RAGGED
            return b

        assert np.array_equal(again().get_cells(), want)
        assert again().population() == int(want.sum())
        assert again().hash() == fresh.hash()
        assert np.array_equal(again().render_gray8(200), fresh.render_gray8(200))
        assert np.array_equal(again().view_counts(3, 5, 8, 100, 30), fresh.view_counts(3, 5, 8, 100, 30))
        assert np.array_equal(again().save_packed(), fresh.save_packed())
        assert again().to_rle() == fresh.to_rle()
        assert np.array_equal(again().get_region(960, 250, 41, 50), want[250:300, 960:1001])


@pytest.mark.parametrize("boundary", [0, 1])
def test_mixed_call_lengths_and_setters(gol, boundary):
    w, h = 1001, 300
    cells = ref.soup(w, h, 13)
    step = lambda c, g: ref.ref_step(c, 0x048, 0x00C, boundary, g)
    with gol.Board(w, h, boundary, rule="B36/S23") as b:
        passes = []
        b.set_cells(cells)
        for g in (32, 3, 32):
            b.step(g)
            passes.append(b.get_option("last_pass"))
        assert passes == [RULE_RAGGED, BYTES, RULE_RAGGED] and b.generation == 67
        assert np.array_equal(b.get_cells(), step(cells, 67))
        b.step(8).step(5)  # two passes running, the state never leaves the scratch rows
        assert np.array_equal(b.get_cells(), step(cells, 80))
        # every setter drops the scratch state: what it wrote is what the next pass packs
        b.step(32).set_cells(cells).step(8)
        assert np.array_equal(b.get_cells(), step(cells, 8))
        b.step(32).clear().step(8)
        assert b.population() == 0 and b.generation == 8
        other = ref.soup(w, h, 14)
        with gol.Board(w, h, boundary) as src:
            snap = src.set_cells(other).save_packed()
        b.step(32).load_packed(snap).step(8)
        assert np.array_equal(b.get_cells(), step(other, 8))
        b.step(32).seed_splitmix(5)
        seeded = b.get_cells()
        assert np.array_equal(b.seed_splitmix(5).step(8).get_cells(), step(seeded, 8))
        b.step(32).seed_dotnet(7)
        seeded = b.get_cells()
        assert np.array_equal(b.seed_dotnet(7).step(8).get_cells(), step(seeded, 8))
        b.step(32).set_states(other).step(8)
        assert np.array_equal(b.get_states(), step(other, 8))
        b.step(32).place_rle("bo$2bo$3o!", 996, 297)  # a point setter modifies the bytes the pass left
        held = b.get_cells()
        assert np.array_equal(b.step(8).get_cells(), step(held, 8))


@pytest.mark.parametrize("boundary", [0, 1])
def test_conway_and_back_between_the_ragged_passes(gol, boundary):
    w, h = 1001, 300
    cells = ref.soup(w, h, 15)
    with gol.Board(w, h, boundary, rule="B36/S23") as b:
        b.set_cells(cells).step(32)
        assert b.get_option("last_pass") == RULE_RAGGED
        now = ref.ref_step(cells, 0x048, 0x00C, boundary, 32)
        b.set_rule("B3/S23").step(32)
        assert b.get_option("last_pass") not in (BYTES, RULE_RAGGED, 1)  # the ragged B3/S23 pass of this size
        now = ref.ref_step(now, 8, 12, boundary, 32)
        b.set_rule("B36/S23").step(32)
        assert b.get_option("last_pass") == RULE_RAGGED
        now = ref.ref_step(now, 0x048, 0x00C, boundary, 32)
        assert np.array_equal(b.get_cells(), now) and b.generation == 96


def test_step_timed_reports_the_pass_and_pass_timing_refuses(gol):
    with gol.Board(1001, 300, rule="B36/S23") as b:
        b.seed_splitmix(3)
        before = b.get_cells()
        assert b.step_timed(32) > 0 and b.get_option("last_pass") == RULE_RAGGED and b.generation == 32
        assert np.array_equal(b.get_cells(), ref.ref_step(before, 0x048, 0x00C, 0, 32))
        with pytest.raises(NotImplementedError):
            b.pass_timing()
