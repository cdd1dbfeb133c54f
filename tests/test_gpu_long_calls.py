"""Single gol_step calls that cross the per-launch generation caps (csrc/gol_passes.cpp ping_pong).

ping_pong splits one call into launches of at most kCoopMaxGensPerLaunch = 32768 generations on the cooperative,
rows-on-lanes and cooperative-ragged passes ("a launch's granule tags count its blocks in 16 bits":
csrc/gol_coop.hip tag_of = epoch << 16 | block + 1) and kResidentMaxGensPerLaunch = 65536 on the single-wave and the
two LDS-resident passes, flips the buffer after every launch and, on the persistent passes, bumps the epoch.  Every
case here is ONE call longer than its pass's cap (and one of exactly the cap): the second and third launches, the
buffer parity they leave for the next call, block numbers up to the cap at a hand-off depth of 1, and a rows-on-lanes
launch shorter than one hand-off block, which only the split can make.

The inputs (tests/long_call_inputs.py; no random soups, which settle and then hide even miscounts) keep changing for
as long as a call lasts, and the oracle's board at generation N costs milliseconds: a gun and eater of period 30 on
both boundaries, a glider on the torus.  Together they miss only miscounts that are multiples of 4 lcm(h, w) and 30
generations at once (1200 at 100 x 100); tests/test_long_call_inputs.py checks that on the reference alone.  Every
case asserts the pass the call took ("last_pass"), the generation counter and the whole board bit for bit.
"""
import numpy as np
import pytest

import long_call_inputs as lci
from long_call_inputs import BOUNDED, TORUS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gol():
    import gameoflifewithactors_amd as g
    from gameoflifewithactors_amd import _lib

    _lib.load()
    return g


INPUTS = ("gun-torus", "gun-bounded", "glider-torus")
ROWS = {row[0]: row for row in lci.LONG_CALLS}


def _input(oracle, kind, w, h):
    """(first board, boundary, n -> expected board at generation n)."""
    if kind == "glider-torus":
        b0 = lci.glider(h, w, w - 2, h - 2)  # it starts across the torus's corner
        return b0, TORUS, lambda n: lci.glider_expected(b0, oracle, n)
    boundary = TORUS if kind == "gun-torus" else BOUNDED
    b0 = lci.gun_eater(h, w)
    return b0, boundary, lambda n: lci.gun_eater_expected(oracle, b0, n, boundary)


CALLS = [(name, n, kind)
         for name, w, h, opts, want, cap, ns, with_glider in lci.LONG_CALLS
         for n in ns for kind in INPUTS if with_glider or kind != "glider-torus"]


@pytest.mark.parametrize("name,n,kind", CALLS, ids=lambda v: str(v))
def test_one_call_across_the_cap(gol, oracle, name, n, kind):
    _, w, h, opts, want_pass, cap, _, _ = ROWS[name]
    b0, boundary, expected = _input(oracle, kind, w, h)
    with gol.Board(w, h, boundary, options=opts) as b:
        b.set_cells(b0)
        lanes_before = b.get_option("lanes_launches")
        b.step(n)
        assert b.get_option("last_pass") == want_pass
        assert b.generation == n
        if want_pass == lci.LANES:
            assert b.get_option("lanes_launches") - lanes_before == lci.launches(n, cap)
        np.testing.assert_array_equal(b.get_cells(), expected(n))


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("name,n", lci.FURTHER_CALLS, ids=lambda v: str(v))
def test_a_further_call_reads_what_the_long_call_left(gol, oracle, name, n, kind):
    """Two launches leave the result in the buffer the call started from, three in the other one: the next call on
    the handle must read the one ping_pong ended on."""
    _, w, h, opts, want_pass, cap, _, _ = ROWS[name]
    assert lci.launches(n, cap) in (2, 3)
    b0, boundary, expected = _input(oracle, kind, w, h)
    with gol.Board(w, h, boundary, options=opts) as b:
        b.set_cells(b0).step(n)
        assert b.get_option("last_pass") == want_pass
        assert b.generation == n
        np.testing.assert_array_equal(b.get_cells(), expected(n))
        b.step(lci.FURTHER)
        assert b.generation == n + lci.FURTHER
        np.testing.assert_array_equal(b.get_cells(), expected(n + lci.FURTHER))


def test_batch_one_long_call(gol, oracle):
    """The batch has no cap: one launch whose loop count is 64 bits wide.  Gun and eater, glider and an empty board,
    70001 generations, then the gun's populations one period and two periods on."""
    w, h, n = lci.BATCH_CALL
    gun0, glider0 = lci.gun_eater(h, w), lci.glider(h, w, w - 2, h - 2)
    want = np.stack([lci.gun_eater_expected(oracle, gun0, n, TORUS), lci.glider_expected(glider0, oracle, n),
                     np.zeros((h, w), np.uint8)])
    with gol.BoardBatch(w, h, 3, TORUS) as bb:
        bb.set_cells(np.stack([gun0, glider0, np.zeros((h, w), np.uint8)]))
        bb.step(n)
        assert bb.generation == n
        np.testing.assert_array_equal(bb.get_cells(), want)
        assert [int(v) for v in bb.hashes()] == [oracle.board_hash(x) for x in want]
        pops = [oracle.population(x) for x in want]
        assert [int(v) for v in bb.populations()] == pops
        assert pops[1:] == [5, 0] and pops[0] > 5
        trace = bb.step_trace(60, every=30)
        assert trace.shape == (2, 3)
        assert [int(v) for v in trace[:, 0]] == [pops[0], pops[0]]  # the gun's period is 30
        assert bb.generation == n + 60
        np.testing.assert_array_equal(bb.get_cells(0, 1)[0], want[0])
        np.testing.assert_array_equal(bb.get_cells(1, 1)[0], lci.glider_expected(glider0, oracle, n + 60))
