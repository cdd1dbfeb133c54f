"""The inputs of tests/test_gpu_long_calls.py (tests/long_call_inputs.py), checked against the oracle alone.

The GPU tests compare one long gol_step call with the oracle's board at a REDUCED generation number (the gun and eater
modulo 30, the glider modulo 4 and rolled).  That is only a test if the reduction is right and if the expected board
at N differs from the expected board at every nearby generation: these conditions, on the reference alone, are what
makes the GPU tests able to fail.  For every board shape, boundary and N those tests use.
"""
import numpy as np
import pytest

import long_call_inputs as lci
from long_call_inputs import BOUNDED, TORUS

# (w, h, boundary) of every gun-and-eater board and (w, h) of every glider board the GPU tests step, with the
# generation counts asked of each
GUN_NS, GLIDER_NS = {}, {}
for _name, _w, _h, _opts, _pass, _cap, _ns, _glider in lci.LONG_CALLS:
    _all = set(_ns) | {n for name, n in lci.FURTHER_CALLS if name == _name}
    for _bd in (TORUS, BOUNDED):
        GUN_NS.setdefault((_w, _h, _bd), set()).update(_all)
    if _glider:
        GLIDER_NS.setdefault((_w, _h), set()).update(_all)
GUN_NS[(lci.BATCH_CALL[0], lci.BATCH_CALL[1], TORUS)].add(lci.BATCH_CALL[2])
GLIDER_NS[lci.BATCH_CALL[:2]].add(lci.BATCH_CALL[2])

GUN_BOARDS = sorted(GUN_NS)
GLIDER_BOARDS = sorted(GLIDER_NS)
SMALLEST = min(GLIDER_BOARDS, key=lambda wh: wh[0] * wh[1])


def seam_glider(h, w):
    """The glider of the GPU tests: it starts across the torus's corner."""
    return lci.glider(h, w, w - 2, h - 2)


@pytest.fixture(scope="module")
def phases(oracle):
    """(w, h, boundary) -> the 31 boards of generations T .. T + 30, stepped one generation at a time."""
    memo = {}

    def get(w, h, boundary):
        if (w, h, boundary) not in memo:
            p = [oracle.c_run(lci.gun_eater(h, w), lci.T, boundary)]
            for _ in range(lci.PERIOD):
                p.append(oracle.c_run(p[-1], 1, boundary))
            memo[w, h, boundary] = p
        return memo[w, h, boundary]

    return get


def test_the_table_names_every_pass_with_a_cap():
    assert {row[4] for row in lci.LONG_CALLS} == {lci.WAVE, lci.LANES, lci.COOP, lci.COOP_RAGGED, lci.RESIDENT}
    for name, w, h, opts, want, cap, ns, with_glider in lci.LONG_CALLS:
        assert cap == (lci.RESIDENT_CAP if want in (lci.WAVE, lci.RESIDENT) else lci.COOP_CAP), name
        assert max(ns) > cap and w >= 64 and h >= 48, name
    names = [row[0] for row in lci.LONG_CALLS]
    assert all(name in names for name, _ in lci.FURTHER_CALLS)
    assert (lci.launches(32768, 32768), lci.launches(32769, 32768), lci.launches(65573, 32768)) == (1, 2, 3)
    assert (lci.launches(65536, 65536), lci.launches(65537, 65536), lci.launches(131073, 65536)) == (1, 2, 3)


@pytest.mark.parametrize("w,h,boundary", GUN_BOARDS)
def test_gun_eater_has_period_30_from_generation_120(phases, w, h, boundary):
    p = phases(w, h, boundary)
    np.testing.assert_array_equal(p[lci.PERIOD], p[0])
    for i in range(lci.PERIOD):
        for j in range(i):
            assert not np.array_equal(p[i], p[j]), f"phases {j} and {i} are the same board"


@pytest.mark.parametrize("w,h,boundary", GUN_BOARDS)
def test_gun_eater_stays_clear_of_the_edges(oracle, phases, w, h, boundary):
    """Rows <= 42 and columns <= 56 over the transient and the whole cycle: the torus and the bounded board agree."""
    b = lci.gun_eater(h, w)
    seen = b.copy()
    for _ in range(lci.T + lci.PERIOD):
        b = oracle.c_run(b, 1, boundary)
        seen |= b
    np.testing.assert_array_equal(b, phases(w, h, boundary)[lci.PERIOD])
    ys, xs = np.nonzero(seen)
    assert ys.max() <= 42 and xs.max() <= 56 and ys.min() >= 1 and xs.min() >= 1
    if boundary == BOUNDED:
        for mine, other in zip(phases(w, h, BOUNDED), phases(w, h, TORUS)):
            np.testing.assert_array_equal(mine, other)


@pytest.mark.parametrize("w,h,boundary", GUN_BOARDS)
def test_gun_eater_expected_is_sensitive_at_every_n(oracle, phases, w, h, boundary):
    """The expected board at N is the cycle's phase (N - T) % 30 and differs from the expected board at N + d for
    every d in -64 .. 64 but 0, +-30 and +-60."""
    p = phases(w, h, boundary)
    b0 = lci.gun_eater(h, w)
    for n in sorted(GUN_NS[w, h, boundary]):
        want = lci.gun_eater_expected(oracle, b0, n, boundary)
        np.testing.assert_array_equal(want, p[(n - lci.T) % lci.PERIOD], err_msg=f"N = {n}")
        for d in range(-64, 65):
            other = p[lci.gun_eater_generation(n + d) - lci.T]
            assert np.array_equal(want, other) == (d in (0, 30, -30, 60, -60)), (n, d)


@pytest.mark.parametrize("w,h", GLIDER_BOARDS)
def test_glider_moves_one_cell_in_4_generations(oracle, w, h):
    b0 = seam_glider(h, w)
    assert b0.sum() == 5
    b = b0
    for _ in range(3):  # the identity holds from any of the glider's 4 phases
        np.testing.assert_array_equal(oracle.c_run(b, 4, TORUS), np.roll(b, (1, 1), (0, 1)))
        b = oracle.c_run(b, 1, TORUS)
    np.testing.assert_array_equal(lci.glider_expected(b0, oracle, 0), b0)
    np.testing.assert_array_equal(lci.glider_expected(b0, oracle, 4 * h * w), b0)


@pytest.mark.parametrize("w,h", GLIDER_BOARDS)
def test_glider_expected_is_sensitive_at_every_n(oracle, w, h):
    """Only d = 0 is exempt: the glider's period on these boards (4 lcm(h, w) >= 256) is beyond +-64."""
    b0 = seam_glider(h, w)
    for n in sorted(GLIDER_NS[w, h]):
        want = lci.glider_expected(b0, oracle, n)
        assert want.sum() == 5
        for d in range(-64, 65):
            assert np.array_equal(want, lci.glider_expected(b0, oracle, n + d)) == (d == 0), (n, d)


def _straight(oracle, b0, n, boundary):
    """n generations one after another: the C oracle on the bounded board, its bit-packed twin (gol_fast.c, pinned to
    it by tests/test_oracle.py) on the torus, where the C oracle takes 6 s for these runs."""
    if boundary == BOUNDED:
        return oracle.c_run(b0, n, boundary)
    return oracle.fast_run(b0, n, boundary, threads=1)[0]


@pytest.mark.parametrize("boundary,n", [(TORUS, 65537), (BOUNDED, 70001)])
def test_gun_eater_expected_equals_a_straight_run(oracle, boundary, n):
    w, h = SMALLEST
    b0 = lci.gun_eater(h, w)
    straight = _straight(oracle, b0, n, boundary)
    np.testing.assert_array_equal(lci.gun_eater_expected(oracle, b0, n, boundary), straight)
    for d in (-2, -1, 1, 2, 8, 16):  # 32768 = 8 and 65536 = 16 (mod 30): a dropped or doubled launch
        assert not np.array_equal(lci.gun_eater_expected(oracle, b0, n + d, boundary), straight), d


def test_glider_expected_equals_a_straight_run(oracle):
    w, h = SMALLEST
    b0 = seam_glider(h, w)
    n = 65573
    straight = _straight(oracle, b0, n, TORUS)
    np.testing.assert_array_equal(lci.glider_expected(b0, oracle, n), straight)
    for d in (-2, -1, 1, 2, 8, 16):
        assert not np.array_equal(lci.glider_expected(b0, oracle, n + d), straight), d


def test_the_two_inputs_together_are_blind_to_multiples_of_1200_only(oracle):
    """On the batch's 100 x 100 torus: the gun repeats every 30 generations, the glider every 400."""
    w, h, n = lci.BATCH_CALL
    assert (w, h) == (100, 100)
    g0 = seam_glider(h, w)
    want = lci.glider_expected(g0, oracle, n)
    same = [d for d in range(1, 1201) if d % 30 == 0 and np.array_equal(want, lci.glider_expected(g0, oracle, n + d))]
    assert same == [1200]
