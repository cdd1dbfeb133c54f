#!/usr/bin/env python
"""Device time of the ensemble cycle census (BoardBatch.cycles, csrc/gol_cycles.hip) beside the plain batch step.

Gliders.  1, 1024 and 16384 boards of the reference's 100 x 100 torus, one glider each, so every wave runs the same
known number of generation steps (steps[i]: 911 in the Brent phase, 400 to B_lambda, none in lockstep).  One census call
with G = 1000 is timed with HIP events on the handle's stream around the kernel (gol_debug_ensemble_cycles_us) after a
warm-up call, --reps times.  The baseline is gol_batch_step_timed -- the batch step's unchanged kernel -- for exactly
steps[0] generations on the same batch in the same session, a baseline call after every census call.

The allowed ratio is not a tuned number; it is the product of two terms, both written out:
  static overhead   the VALU instructions the census adds per generation step (per word one v_bitop3 for d | (a ^ b);
                    the v_cmp of the ballot; the v_cmp / v_readfirstlane of the window test) against those of one
                    wave_generation, both counted in the 100 x 100 torus kernels' disassembly (COMPARE_VALU, GEN_VALU),
                    weighted by the steps that carry a compare (the Brent phase's; the steps to B_lambda carry none)
  baseline spread   max / min of the baseline's own repetitions
A measured ratio above their product is reported as such (meets_margin false), not hidden.

Soups.  1024 boards, dotnet-mod2, board i <- seed i, G = 5000: the real workload; its time and the distribution of
(transient, period) go into the result.

    python tools/cycles_bench.py [--out profiles/cycles/cycles_bench.json] [--reps 7]
"""
import argparse
import collections
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gameoflifewithactors_amd import BoardBatch, _lib  # noqa: E402

W = H = 100
COUNTS = (1, 1024, 16384)
G_GLIDER, G_SOUP, SOUPS = 1000, 5000, 1024
GLIDER = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], np.uint8)
# gol_batch_cycles<4, 2, false> / gol_batch_step<4, 2, false, false>, hipcc -O3 --offload-arch=gfx950: VALU instructions
# of one wave_generation (the same 96 in both kernels' loops, beside 16 ds_bpermute) and those the compare adds
GEN_VALU, COMPARE_VALU = 96, 11
KERNEL = {"vgprs": 55, "scratch_bytes": 0, "occupancy_waves_per_simd": 8,
          "vgprs_128x256": 84, "occupancy_128x256": 5}


def stats(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2), "max_us": round(max(us), 2)}


def census_us(lib, b, G):
    res = b.cycles(G, with_steps=True)
    us = ctypes.c_double()
    _lib.check(lib.gol_debug_ensemble_cycles_us(b._h, ctypes.byref(us)), "gol_debug_ensemble_cycles_us")
    return res, us.value


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cycles", "cycles_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    lib = _lib.load()
    result = {"board": [W, H], "boundary": "torus", "reps": a.reps,
              "timing": "HIP events on the handle's stream around the kernel (gol_debug_ensemble_cycles_us / "
                        "gol_batch_step_timed), one warm-up call first, a baseline call after every census call",
              "kernel": dict(KERNEL, generation_valu=GEN_VALU, compare_valu=COMPARE_VALU), "gliders": {}}
    one = np.zeros((H, W), np.uint8)
    one[3:6, 1:4] = GLIDER
    for count in COUNTS:
        with BoardBatch(W, H, count) as b:
            for first in range(0, count, 1024):
                b.set_cells(np.broadcast_to(one, (min(1024, count - first), H, W)), first=first)
            (mu, lam, pop, steps), _ = census_us(lib, b, G_GLIDER)  # the warm-up call
            if not ((mu == 0).all() and (lam == 400).all() and (pop == 5).all() and (steps == steps[0]).all()):
                print(f"count {count}: a glider board is not (0, 400, 5)", file=sys.stderr)
                return 1
            n = int(steps[0])
            with_compare = n - 400  # the Brent phase; the 400 steps to B_lambda compare nothing
            b.step_timed(n)
            census, base = [], []
            for _ in range(a.reps):
                census.append(census_us(lib, b, G_GLIDER)[1])
                base.append(b.step_timed(n))
            static = (with_compare * (GEN_VALU + COMPARE_VALU) + (n - with_compare) * GEN_VALU) / (n * GEN_VALU)
            spread = max(base) / min(base)
            ratio = statistics.median(census) / statistics.median(base)
            case = {"steps_per_board": n, "steps_with_compare": with_compare, "census": stats(census),
                    "baseline_step_timed": stats(base), "us_per_step": round(statistics.median(census) / n, 4),
                    "ratio": round(ratio, 4), "static_overhead": round(static, 4), "baseline_spread": round(spread, 4),
                    "margin": round(static * spread, 4), "meets_margin": bool(ratio <= static * spread)}
            result["gliders"][str(count)] = case
            print(count, json.dumps(case), flush=True)
    with BoardBatch(W, H, SOUPS) as b:
        b.seed_dotnet(list(range(SOUPS)))
        census_us(lib, b, G_SOUP)  # warm-up
        runs = [census_us(lib, b, G_SOUP) for _ in range(a.reps)]
        (mu, lam, pop, steps) = runs[0][0]
        ok = mu >= 0
        q = (lambda v, p: int(np.percentile(v, p))) if ok.any() else (lambda v, p: None)
        result["soups"] = {
            "boards": SOUPS, "init": "dotnet-mod2, board i <- seed i", "max_generations": G_SOUP,
            "census": stats([us for _, us in runs]), "resolved": int(ok.sum()), "unresolved": int((~ok).sum()),
            "periods": {str(k): v for k, v in sorted(collections.Counter(lam[ok].tolist()).items())},
            "transient": {"min": q(mu[ok], 0), "p10": q(mu[ok], 10), "median": q(mu[ok], 50), "p90": q(mu[ok], 90),
                          "max": q(mu[ok], 100)},
            "population_at_transient": {"min": q(pop[ok], 0), "median": q(pop[ok], 50), "max": q(pop[ok], 100)},
            "steps": {"min": int(steps.min()), "median": int(np.median(steps)), "max": int(steps.max()),
                      "bound_6G": 6 * G_SOUP, "sum": int(steps.sum())},
            "board_steps_per_s": round(float(steps.sum()) / (statistics.median([us for _, us in runs]) * 1e-6), 1)}
        print("soups", json.dumps(result["soups"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
