#!/usr/bin/env python
"""Device time of the batch step under a life-like rule (csrc/gol_batch.hip, the rule-table family) beside the B3/S23
kernel the batch always ran.

Soups.  1, 1024 and 16384 boards of the reference's 100 x 100 torus, dotnet-mod2, board i <- seed i.  One call of 1000
generations is timed with HIP events on the handle's stream (gol_batch_step_timed) after a warm-up call, --reps times.
The baseline is the same batch under B3/S23 on the default path -- the parent's unchanged kernel: the disassembly of
the Conway instantiations is identical before and after rules -- one baseline call after every
measured call.  Measured: B3/S23 forced through the table family (gol_debug_batch_rule_table), B36/S23, B3678/S34678.
A step's time does not depend on the cells, so every call steps whatever the previous one left.

The allowed ratio is not a tuned number; for each rule it is the product of two terms, both written out:
  static VALU ratio  the vector instructions of one generation on the path the rule's set bits take through
                     gol_batch_step<4, 2, false, false, uint32_t> (TABLE_FIXED_VALU + TABLE_VALU_PER_BIT per set bit),
                     against those of gol_batch_step<4, 2, false, false> (GEN_VALU), both counted in the disassembly
  baseline spread    max / min of the baseline's own repetitions
A measured ratio above their product is reported as such ("above", with the excess), not hidden.

Census.  1024 soups, B36/S23, G = 5000: the time, the resolved count and the period histogram, beside the Conway
figures of profiles/cycles/cycles_bench.json.

    python tools/rules_bench.py [--out profiles/rules/rules_bench.json] [--reps 7]
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
GENERATIONS, G_SOUP, SOUPS = 1000, 5000, 1024
MEASURED = (("B3/S23", True), ("B36/S23", False), ("B3678/S34678", False))  # (rule, forced through the table family)
CENSUS_RULE = "B36/S23"
# hipcc -O3 --offload-arch=gfx950, the NW 4, RPL 2 torus instantiations of gol_batch_step: VALU instructions of one
# generation.  Conway: 96 (beside 16 ds_bpermute).  Table: 121 whatever the rule (40 of row sums and exchange masks, 9
# per word of planes and qualifiers, 8 zeroed accumulators, the last-word mask) and 16 for each set bit (2 per word),
# walked through the 36 scalar branches of the loop for each rule below.
GEN_VALU, TABLE_FIXED_VALU, TABLE_VALU_PER_BIT = 96, 121, 16
KERNEL = {"step_vgprs": 61, "step_waves_per_simd": 8, "step_vgprs_128x256": 80, "step_waves_per_simd_128x256": 6,
          "cycles_vgprs": 70, "cycles_waves_per_simd": 7, "cycles_vgprs_128x256": 94, "cycles_waves_per_simd_128x256": 5,
          "scratch_bytes": 0}


def stats(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2), "max_us": round(max(us), 2)}


def table_valu(rule):
    birth, survive = _lib.rule_parse(rule)
    return TABLE_FIXED_VALU + TABLE_VALU_PER_BIT * (bin(birth).count("1") + bin(survive).count("1"))


def force_table(lib, b, force):
    _lib.check(lib.gol_debug_batch_rule_table(b._h, force), "gol_debug_batch_rule_table")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rules", "rules_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    lib = _lib.load()
    result = {"board": [W, H], "boundary": "torus", "init": "dotnet-mod2, board i <- seed i", "reps": a.reps,
              "generations_per_call": GENERATIONS,
              "timing": "HIP events on the handle's stream (gol_batch_step_timed), one warm-up call of each kind first, "
                        "a baseline call (B3/S23, default path) after every measured call",
              "kernel": dict(KERNEL, generation_valu=GEN_VALU, table_fixed_valu=TABLE_FIXED_VALU,
                             table_valu_per_set_bit=TABLE_VALU_PER_BIT), "step": {}}
    for count in COUNTS:
        with BoardBatch(W, H, count) as b:
            b.seed_dotnet(list(range(count)))
            result["step"][str(count)] = rows = {}
            for rule, forced in MEASURED:
                def measured():
                    force_table(lib, b, int(forced))
                    us = b.set_rule(rule).step_timed(GENERATIONS)
                    force_table(lib, b, 0)
                    return us

                def baseline():
                    return b.set_rule("B3/S23").step_timed(GENERATIONS)

                measured()
                baseline()
                got, base = [], []
                for _ in range(a.reps):
                    got.append(measured())
                    base.append(baseline())
                static = table_valu(rule) / GEN_VALU
                spread = max(base) / min(base)
                ratio = statistics.median(got) / statistics.median(base)
                margin = static * spread
                row = {"forced_table": forced, "valu_per_generation": table_valu(rule), "measured": stats(got),
                       "baseline_b3s23": stats(base), "ratio": round(ratio, 4), "static_valu_ratio": round(static, 4),
                       "baseline_spread": round(spread, 4), "margin": round(margin, 4),
                       "verdict": "within" if ratio <= margin else "above",
                       "excess": round(max(ratio / margin - 1, 0.0), 4)}
                rows[rule + (" (table)" if forced else "")] = row
                print(count, rule, json.dumps(row), flush=True)
    with BoardBatch(W, H, SOUPS, rule=CENSUS_RULE) as b:
        b.seed_dotnet(list(range(SOUPS)))

        def census():
            res = b.cycles(G_SOUP, with_steps=True)
            us = ctypes.c_double()
            _lib.check(lib.gol_debug_ensemble_cycles_us(b._h, ctypes.byref(us)), "gol_debug_ensemble_cycles_us")
            return res, us.value

        census()  # warm-up
        runs = [census() for _ in range(a.reps)]
        (mu, lam, pop, steps) = runs[0][0]
        ok = mu >= 0
        q = (lambda v, p: int(np.percentile(v, p))) if ok.any() else (lambda v, p: None)
        times = [us for _, us in runs]
        result["census"] = {
            "rule": CENSUS_RULE, "boards": SOUPS, "max_generations": G_SOUP, "census": stats(times),
            "resolved": int(ok.sum()), "unresolved": int((~ok).sum()),
            "periods": {str(k): v for k, v in sorted(collections.Counter(lam[ok].tolist()).items())},
            "transient": {"min": q(mu[ok], 0), "p10": q(mu[ok], 10), "median": q(mu[ok], 50), "p90": q(mu[ok], 90),
                          "max": q(mu[ok], 100)},
            "population_at_transient": {"min": q(pop[ok], 0), "median": q(pop[ok], 50), "max": q(pop[ok], 100)},
            "steps": {"min": int(steps.min()), "median": int(np.median(steps)), "max": int(steps.max()),
                      "bound_6G": 6 * G_SOUP, "sum": int(steps.sum())},
            "board_steps_per_s": round(float(steps.sum()) / (statistics.median(times) * 1e-6), 1)}
        print("census", json.dumps(result["census"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
