#!/usr/bin/env python
"""One rule per board of a batch (gol_ensemble_set_rules): what the per-board table costs, and a rule
map.

(a) Cost of the table.  1, 1024 and 16384 boards of the reference's 100 x 100 torus, dotnet-mod2, board i <- seed i
(the geometries of tools/rules_bench.py).  One call of 1000 generations is timed with HIP events on the handle's stream
(gol_batch_step_timed): the batch under set_rules with the same rule for every board -- the per-board family, each wave
loading its rule from the table -- against the same batch under set_rule with that rule -- the uniform table family,
the rule a kernel argument.  The two differ by one scalar load per wave and launch, so the expectation is a ratio
within the run-to-run spread of 1.0; nothing gates on it.  One warm-up call of each kind, then --reps interleaved pairs.
B3/S23 runs life_next under set_rule, which is another loop altogether, so for it the uniform side is forced through
the table family (gol_debug_batch_rule_table).  A step's time does not depend on the cells, so every call steps whatever
the previous one left.

(b) A rule map.  All 2^18 life-like rules on one 32 x 32 torus soup (gol_batch_seed_dotnet with the same seed for every
board), board i under birth = i & 0x1FF, survive = i >> 9: one gol_ensemble_cycles launch, its device time
(gol_debug_ensemble_cycles_us), the resolved count and the most frequent periods.

    python tools/rule_map_bench.py [--out profiles/rule_map/rule_map_bench.json] [--reps 7]
"""
import argparse
import collections
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gameoflifewithactors_amd import BoardBatch, _lib  # noqa: E402

W = H = 100
COUNTS = (1, 1024, 16384)
GENERATIONS = 1000
MEASURED = (("B3/S23", True), ("B36/S23", False), ("B3678/S34678", False))  # (rule, uniform side forced to the table)
MAP_W = MAP_H = 32
MAP_SEED, MAP_G, MAP_BOARDS = 12345, 1000, 1 << 18


def stats(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2), "max_us": round(max(us), 2)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rule_map", "rule_map_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    lib = _lib.load()
    result = {"reps": a.reps,
              "table_cost": {"board": [W, H], "boundary": "torus", "init": "dotnet-mod2, board i <- seed i",
                             "generations_per_call": GENERATIONS,
                             "timing": "HIP events on the handle's stream (gol_batch_step_timed), one warm-up call of "
                                       "each kind first, a uniform call (set_rule) after every per-board call "
                                       "(set_rules)",
                             "step": {}}}
    for count in COUNTS:
        with BoardBatch(W, H, count) as b:
            b.seed_dotnet(list(range(count)))
            result["table_cost"]["step"][str(count)] = rows = {}
            for rule, forced in MEASURED:
                masks = np.array([_lib.rule_parse(rule)] * count, np.int64)

                def per_board():
                    return b.set_rules(masks).step_timed(GENERATIONS)

                def uniform():
                    _lib.check(lib.gol_debug_batch_rule_table(b._h, int(forced)), "gol_debug_batch_rule_table")
                    us = b.set_rule(rule).step_timed(GENERATIONS)
                    _lib.check(lib.gol_debug_batch_rule_table(b._h, 0), "gol_debug_batch_rule_table")
                    return us

                per_board()
                uniform()
                got, base = [], []
                for _ in range(a.reps):
                    got.append(per_board())
                    base.append(uniform())
                ratio = statistics.median(got) / statistics.median(base)
                spread = max(max(base) / min(base), max(got) / min(got))
                row = {"uniform_forced_table": forced, "per_board_table": stats(got), "uniform_rule": stats(base),
                       "ratio": round(ratio, 4), "spread": round(spread, 4),
                       "verdict": "within the spread" if abs(ratio - 1) <= spread - 1 else
                                  ("above the spread" if ratio > 1 else "below the spread")}
                rows[rule] = row
                print(count, rule, json.dumps(row), flush=True)

    with BoardBatch(MAP_W, MAP_H, MAP_BOARDS) as b:
        t0 = time.perf_counter()
        b.seed_dotnet([MAP_SEED] * MAP_BOARDS)
        seed_s = time.perf_counter() - t0
        i = np.arange(MAP_BOARDS, dtype=np.int64)
        t0 = time.perf_counter()
        b.set_rules(np.stack([i & 0x1FF, i >> 9], 1))
        set_rules_s = time.perf_counter() - t0

        def census():
            t0 = time.perf_counter()
            res = b.cycles(MAP_G, with_steps=True)
            wall = time.perf_counter() - t0
            us = ctypes.c_double()
            _lib.check(lib.gol_debug_ensemble_cycles_us(b._h, ctypes.byref(us)), "gol_debug_ensemble_cycles_us")
            return res, us.value, wall

        census()  # warm-up
        runs = [census() for _ in range(a.reps)]
        mu, lam, pop, steps = runs[0][0]
        ok = mu >= 0
        times = [us for _, us, _ in runs]
        periods = collections.Counter(lam[ok].tolist())
        result["rule_map"] = {
            "board": [MAP_W, MAP_H], "boundary": "torus", "init": "dotnet-mod2, seed %d for every board" % MAP_SEED,
            "rules": "board i: birth = i & 0x1FF, survive = i >> 9", "boards": MAP_BOARDS, "max_generations": MAP_G,
            "launch": stats(times), "call_wall_s": round(statistics.median(w for _, _, w in runs), 4),
            "seed_s": round(seed_s, 3), "set_rules_s": round(set_rules_s, 4),
            "resolved": int(ok.sum()), "unresolved": int((~ok).sum()), "distinct_periods": len(periods),
            "most_frequent_periods": {str(k): v for k, v in periods.most_common(8)},
            "longest_period": int(lam.max()), "longest_transient": int(mu.max()),
            "dies_out": int((ok & (pop == 0)).sum()),
            "steps": {"min": int(steps.min()), "median": int(np.median(steps)), "max": int(steps.max()),
                      "bound_6G": 6 * MAP_G, "sum": int(steps.sum())},
            "board_steps_per_s": round(float(steps.sum()) / (statistics.median(times) * 1e-6), 1)}
        print("rule map", json.dumps(result["rule_map"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
