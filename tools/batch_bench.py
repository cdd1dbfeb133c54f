#!/usr/bin/env python
"""Device time of the batch handle (BoardBatch, csrc/gol_batch.hip) beside the single board it multiplies.

The reference's 100 x 100 torus, dotnet-mod2, board i seeded with seed i.  For count in 1, 64, 256, 1024, 4096 and 16384
one call of 1000 generations is timed with HIP events on the batch's stream (gol_batch_step_timed) after a warm-up call,
--reps times, for both workgroup shapes (one board per 64-thread workgroup, four per 256-thread workgroup).  IN THE SAME
PROCESS one ordinary Board(100, 100) is stepped 1000 generations with step_timed (the single-wave pass: what a caller
had before the batch handle) -- the baseline of every ratio.  After the warm-up call the hashes of at least 8 boards per
count (all of them below 8) are compared with single Boards run from the same seeds; a mismatch exits non-zero.

    python tools/batch_bench.py [--out profiles/batch/batch_bench.json] [--reps 7] [--generations 1000]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gameoflifewithactors_amd import Board, BoardBatch, _lib  # noqa: E402

W = H = 100
COUNTS = (1, 64, 256, 1024, 4096, 16384)
SHAPES = {"wg64": 1, "wg256": 4}  # boards (waves) per workgroup
GATE_ONE, GATE_1024 = 1.10, 2.0   # batch of 1 and of 1024 against the single board (device time ratios)


def stats(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2), "max_us": round(max(us), 2)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "batch_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--generations", type=int, default=1000)
    a = ap.parse_args()
    g = a.generations
    lib = _lib.load()
    result = {"board": [W, H], "boundary": "torus", "init": "dotnet-mod2, board i <- seed i", "generations": g,
              "reps": a.reps, "timing": "HIP events on the handle's stream (gol_step_timed / gol_batch_step_timed), one "
              "warm-up call first", "single_board": {}, "counts": {}}

    want_hash = {}  # seed -> hash of a single Board after g generations

    def single_hash(seed):
        if seed not in want_hash:
            with Board(W, H) as b:
                want_hash[seed] = b.seed_dotnet(seed).step(g).hash()
        return want_hash[seed]

    def time_single():
        with Board(W, H) as b:
            b.seed_dotnet(0).step(g)
            b.synchronize()
            return [b.step_timed(g) for _ in range(a.reps)]

    single = time_single()
    for count in COUNTS:
        sample = sorted(set(list(range(min(4, count))) + [count // 2, count // 3] +
                            list(range(max(0, count - 4), count))))
        case = {"hash_sample": sample}
        with BoardBatch(W, H, count) as b:
            for shape, waves in SHAPES.items():
                _lib.check(lib.gol_debug_batch_group_waves(b._h, waves), "gol_debug_batch_group_waves")
                b.seed_dotnet(list(range(count))).step(g)  # the warm-up call
                hashes = b.hashes()
                bad = [i for i in sample if int(hashes[i]) != single_hash(i)]
                if bad:
                    print(f"count {count} {shape}: boards {bad} differ from single Boards after {g} generations",
                          file=sys.stderr)
                    return 1
                us = [b.step_timed(g) for _ in range(a.reps)]
                med = statistics.median(us)
                case[shape] = dict(stats(us), us_per_generation=round(med / g, 4),
                                   board_generations_per_s=round(count * g / (med * 1e-6), 1),
                                   gcups=round(count * W * H * g / med / 1e3, 2))
        case["wg256_over_wg64"] = round(case["wg256"]["median_us"] / case["wg64"]["median_us"], 4)
        result["counts"][str(count)] = case
        print(count, json.dumps(case), flush=True)
    single += time_single()  # the baseline again after the batches: both halves of the session count
    result["single_board"] = dict(stats(single), gcups=round(W * H * g / statistics.median(single) / 1e3, 3),
                                  path="Board(100, 100).step_timed: the single-wave pass on the byte board")
    base = statistics.median(single)
    default = "wg64"
    r1 = result["counts"]["1"][default]["median_us"] / base
    r1024 = result["counts"]["1024"][default]["median_us"] / base
    result["default_shape"] = default
    result["ratios"] = {"batch_of_1_over_single": round(r1, 4), "gate_batch_of_1": GATE_ONE,
                        "batch_of_1_meets_gate": bool(r1 <= GATE_ONE),
                        "batch_of_1024_over_single": round(r1024, 4), "gate_batch_of_1024": GATE_1024,
                        "batch_of_1024_meets_gate": bool(r1024 <= GATE_1024),
                        "boards_worth_of_single_throughput_at_1024": round(1024 / r1024, 1)}
    print("single_board", json.dumps(result["single_board"]), flush=True)
    print("ratios", json.dumps(result["ratios"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
