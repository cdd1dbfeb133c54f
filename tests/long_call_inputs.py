"""Inputs whose board at generation n is known for any n -- test infrastructure only, a plain helper module.

A random soup settles into still lifes and blinkers within a few thousand generations, and from then on a test that
compares it with the oracle cannot tell n generations from n - 2.  The two inputs here stay sensitive to the exact
generation count for as long as a call lasts, and their expected board costs the oracle at most T + 29 generations:

* `gun_eater`: the oracle's Gosper gun (`GOSPER_GUN` at (2, 2)) with an eater 1 in its glider stream at (53, 39).
  From generation T = 120 the board has period exactly 30 with 30 distinct phases; live cells stay within rows <= 42
  and columns <= 56, so on any board of at least 64 x 48 (w x h) nothing reaches an edge and torus and bounded boards
  agree.  `gun_eater_expected` is the oracle's board at generation T + (n - T) % 30.
* `glider`: the oracle's `GLIDER` on a torus.  After 4 generations it is itself moved one cell down and right, so
  `glider_expected` is the oracle's board at generation n % 4 rolled by n // 4; on an h x w torus the period is
  4 lcm(h, w).  It gets a board of its own: on a square torus its diagonal meets the gun.

tests/test_long_call_inputs.py checks all of this against straight oracle runs, on the CPU.

BLIND SET.  A miscount of d generations goes unseen by the gun alone exactly when d is a multiple of 30 (so 32768 = 8
and 65536 = 16 mod 30, a dropped or doubled launch of either cap, show), by the glider alone when d is a multiple of
4 lcm(h, w), and by both together only when d is a multiple of their least common multiple: 1200 generations on a
100 x 100 torus, 3840 at 64 x 64, 15360 at 256 x 256.
"""
from __future__ import annotations

import numpy as np

import gol_oracle as _o

EATER = "2o$obo$2bo$2b2o!"  # eater 1
T = 120       # first generation of the gun-and-eater cycle used here (the first glider has been eaten)
PERIOD = 30   # the gun's


# the library's enum class Pass (csrc/gol_board.h), as the "last_pass" option reports it
WAVE, LANES, COOP, COOP_RAGGED, RESIDENT = 1, 2, 3, 4, 7
TORUS, BOUNDED = 0, 1

COOP_CAP = 32768      # csrc/gol_passes.cpp kCoopMaxGensPerLaunch
RESIDENT_CAP = 65536  # csrc/gol_passes.cpp kResidentMaxGensPerLaunch

# The long calls of tests/test_gpu_long_calls.py: (name, w, h, board options, pass, its cap, generations of the one
# call, glider too).  The boards are the smallest the suite shows each pass taking (tests/test_gpu_pass_choice.py,
# test_gpu_resident.py); 129 x 300 holds the gun but is stepped with it alone.
_RES = {"coop": 0, "wave_resident": 0}
LONG_CALLS = [
    ("wave-bytes", 100, 100, {}, WAVE, RESIDENT_CAP, (65536, 65537, 70001), True),
    ("wave-packed", 64, 64, {}, WAVE, RESIDENT_CAP, (65537, 70001), True),
    ("resident-packed", 64, 64, _RES, RESIDENT, RESIDENT_CAP, (65537, 70001), True),
    ("resident-bytes", 100, 100, {"resident_max_cells": 1 << 20, **_RES}, RESIDENT, RESIDENT_CAP, (65537,), True),
    ("coop", 256, 256, {"lanes": 0}, COOP, COOP_CAP, (32768, 32769, 65573), True),
    # a hand-off per generation: block numbers up to the cap itself
    ("coop-k1", 256, 256, {"lanes": 0, "coop_k": 1}, COOP, COOP_CAP, (32768, 32769, 65573), True),
    # the cap is no multiple of the depth: every full launch ends on a short block
    ("coop-k3", 256, 256, {"lanes": 0, "coop_k": 3}, COOP, COOP_CAP, (32768, 32769, 65573), True),
    # 32769: a lanes launch of one generation; 65573: three launches, the last block short
    ("lanes", 256, 256, {}, LANES, COOP_CAP, (32768, 32769, 65573), True),
    ("coop-ragged", 129, 300, {}, COOP_RAGGED, COOP_CAP, (32769, 65573), False),
]
# A further call of FURTHER generations on the handle a long call left (name of the row above, generations of the
# long call): two launches and three launches of either cap.
FURTHER = 7
FURTHER_CALLS = [("coop", 32769), ("coop", 65573), ("lanes", 32769), ("lanes", 65573),
                 ("wave-packed", 65537), ("wave-packed", 131073)]
BATCH_CALL = (100, 100, 70001)  # (w, h, generations) of the batch's one call


def launches(n: int, cap: int) -> int:
    """Launches gol_step splits a call of n generations into on a pass of that cap."""
    return -(-n // cap)


def gun_eater(h: int, w: int) -> np.ndarray:
    """(h, w) uint8 board (w >= 64, h >= 48): Gosper gun at (2, 2), eater 1 at (53, 39)."""
    if w < 64 or h < 48:
        raise ValueError("gun_eater needs a board of at least 64 x 48 (w x h)")
    b = np.zeros((h, w), np.uint8)
    _o.place_rle(b, _o.GOSPER_GUN, 2, 2)
    _o.place_rle(b, EATER, 53, 39)
    return b


def gun_eater_generation(n: int) -> int:
    """The generation in [T, T + PERIOD) whose board generation n >= T repeats."""
    if n < T:
        raise ValueError(f"the cycle starts at generation {T}")
    return T + (n - T) % PERIOD


def gun_eater_expected(oracle, b0: np.ndarray, n: int, boundary: int) -> np.ndarray:
    """Board b0 = gun_eater(h, w) after n >= T generations."""
    return oracle.c_run(b0, gun_eater_generation(n), boundary)


def glider(h: int, w: int, x: int, y: int) -> np.ndarray:
    """(h, w) uint8 board holding one glider, its bounding box's corner at column x, row y; torus only."""
    return _o.place_rle(np.zeros((h, w), np.uint8), _o.GLIDER, x, y)


def glider_expected(b0: np.ndarray, oracle, n: int) -> np.ndarray:
    """Board b0 = glider(h, w, x, y) after n generations on the torus."""
    return np.roll(oracle.c_run(b0, n % 4, 0), (n // 4, n // 4), (0, 1))
