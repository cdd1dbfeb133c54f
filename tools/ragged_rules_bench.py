#!/usr/bin/env python
"""Device time of a ragged board (width not a multiple of 32) under a life-like and a Generations rule on the ragged
streaming passes (gol_rule_stream_ragged / gol_gen_stream_ragged on whole-word scratch rows) beside

  bytes     the same board with board option "rule_ragged" 0: the per-generation byte step, what such a board ran
            before the passes existed and the thing they are measured against;
  aligned   the ilv-1 packed board of width 32 * ceil(W / 32) and the same height on the rule / Generations streaming
            pass: what the ragged loads, masks and the scratch rows cost (reported, not gated).

The ragged legs run with board option "rule_ragged" 2, so every cell is measured whatever the library's thresholds are;
"default_takes" says whether a board with default options takes the pass for that call (gol_policy.cpp use_rule_ragged).
The ragged pass is timed twice: "ragged", call after call with the state resident in the scratch rows, and
"ragged_cold", every call preceded by a readback (gol_population) that brings the bytes up to date, so that the timed
call packs the board again -- the cost the call-length threshold (gol_policy.cpp kRuleRaggedMinGens) has to cover.

gol_seed_splitmix, HIP events on the board's stream (gol_step_timed), one warm-up call of each leg and --reps
repetitions, the legs interleaved within a repetition.  Each shape runs as a process of its own under its own time
limit, and a shape that fails ends the run.  Per cell (shape, boundary, rule, call length): the medians, the ratios, and
"faster" where the resident median is below the byte step's -- the requirement for every cell the default takes; the
cells where the call with the pack is above the byte step are listed beside it.

    python tools/ragged_rules_bench.py [--out profiles/ragged_rules/ragged_rules_bench.json] [--reps 7]
    python tools/ragged_rules_bench.py --shape 1001      (one shape, in this process; merges into --out)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1001, 1001, 240), (10001, 10001, 300), (14189, 14189, 420))  # (W, H, time limit s); 14189^2 >= 3 * 2^26
RULES = ("B36/S23", "B2/S345/4")
CALLS = (4, 16, 64)


def policy_min_gens():
    """kRuleRaggedMinGens as gol_policy.cpp has it: every call length here must be at least that."""
    import re

    with open(os.path.join(ROOT, "gameoflifewithactors_amd", "csrc", "gol_policy.cpp")) as f:
        return int(re.search(r"constexpr int64_t kRuleRaggedMinGens = (\d+);", f.read()).group(1))


MIN_GENS = policy_min_gens()
assert min(CALLS) >= MIN_GENS, (CALLS, MIN_GENS)
RULE_RAGGED, GEN_RAGGED, BYTES, RULE_STREAM, GEN_STREAM = 13, 14, 8, 11, 12  # gol::Pass (csrc/gol_board.h)


def stats(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2), "max_us": round(max(us), 2)}


def one_shape(w, h, reps):
    from gameoflifewithactors_amd import Board

    wa = 32 * -(-w // 32)
    cells = {}
    for boundary in (0, 1):
        for rule in RULES:
            gen = rule.count("/") == 2
            with Board(w, h, boundary, rule=rule, options={"rule_ragged": 2}) as new, \
                    Board(w, h, boundary, rule=rule, options={"rule_ragged": 0}) as old, \
                    Board(wa, h, boundary, ilv=1, rule=rule) as al:
                for b in (new, old, al):
                    b.seed_splitmix(0x5EED)
                with Board(w, h, boundary, rule=rule) as dflt:  # what the default options choose, per call length
                    takes = {g: dflt.seed_splitmix(0x5EED).step(g).get_option("last_pass") in (RULE_RAGGED, GEN_RAGGED)
                             for g in CALLS}
                legs = {"ragged": lambda g: new.step_timed(g), "ragged_cold": lambda g: (new.population(), new.step_timed(g))[1],
                        "bytes": lambda g: old.step_timed(g), "aligned": lambda g: al.step_timed(g)}
                for gens in CALLS:
                    got = {k: [] for k in legs}
                    for rep in range(reps + 1):  # the first repetition warms every leg up
                        for k, call in legs.items():
                            us = call(gens)
                            if rep:
                                got[k].append(us)
                    passes = (new.get_option("last_pass"), old.get_option("last_pass"), al.get_option("last_pass"))
                    assert passes == (GEN_RAGGED if gen else RULE_RAGGED, BYTES, GEN_STREAM if gen else RULE_STREAM), passes
                    med = {k: statistics.median(v) for k, v in got.items()}
                    row = {k: stats(v) for k, v in got.items()}
                    row.update(us_per_generation={k: round(v / gens, 3) for k, v in med.items()},
                               bytes_over_ragged=round(med["bytes"] / med["ragged"], 2),
                               bytes_over_ragged_cold=round(med["bytes"] / med["ragged_cold"], 2),
                               ragged_over_aligned=round(med["ragged"] / med["aligned"], 3),
                               default_takes=takes[gens],
                               verdict="faster" if med["ragged"] < med["bytes"] else "slower",
                               verdict_cold="faster" if med["ragged_cold"] < med["bytes"] else "slower")
                    key = f"{'bounded' if boundary else 'torus'} {rule} {gens}"
                    cells[key] = row
                    print(w, h, key, json.dumps(row), flush=True)
    return {"aligned_width": wa, "cells": cells}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_rules", "ragged_rules_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shape", type=int, default=0)
    a = ap.parse_args()
    if a.shape:
        w, h = {s[0]: s[:2] for s in SHAPES}[a.shape]
        result = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                result = json.load(f)
        result.setdefault("shapes", {})[f"{w}x{h}"] = one_shape(w, h, a.reps)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"init": "gol_seed_splitmix(0x5EED)", "reps": a.reps, "rules": RULES, "calls": CALLS, "min_gens": MIN_GENS,
                   "timing": "HIP events on the board's stream (gol_step_timed), one warm-up call of each leg first, the "
                             "legs interleaved within a repetition; ragged_cold: a readback before every call, so the "
                             "call packs the board again",
                   "shapes": {}}, f, indent=1)
    for w, _, limit in SHAPES:  # a process and a time limit per shape; the first that fails ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--shape",
                             str(w), "--out", a.out, "--reps", str(a.reps)]).returncode
        if rc != 0:
            print(f"shape {w}: exit status {rc}; stopping", flush=True)
            return rc
    with open(a.out) as f:
        result = json.load(f)
    taken = [(f"{s} {k}", c) for s, v in result["shapes"].items() for k, c in v["cells"].items() if c["default_takes"]]
    slow = [k for k, c in taken if c["verdict"] != "faster"]
    result["requirement"] = {"text": "ragged median below bytes in every cell the default options take",
                             "met": not slow, "slower_cells": slow,
                             "slower_with_the_pack_in_the_call": [k for k, c in taken if c["verdict_cold"] != "faster"],
                             "not_taken_by_default": [f"{s} {k}" for s, v in result["shapes"].items()
                                                      for k, c in v["cells"].items() if not c["default_takes"]]}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("requirement", json.dumps(result["requirement"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
