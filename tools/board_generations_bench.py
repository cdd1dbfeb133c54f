#!/usr/bin/env python
"""Device time of a single board under a Generations rule (gol_set_generations_rule: the multi-plane streaming pass
csrc/gol_gen_stream.hip) beside the same board under the same B.../S... at two states -- the rule-generic streaming
pass csrc/gol_rule_step.hip, the parent's unchanged kernels (profiles/board_generations/).

Torus, gol_seed_splitmix, HIP events on the board's stream (gol_step_timed), one warm-up call of each kind and --reps
repetitions, one baseline call after every measured call.  Measured: B2/S345 at nstates 3, 4 and 8 (1, 2 and 3 decay
planes).  A step's time does not depend on the cells, so every call steps whatever the previous one left.  Where the
depth table (csrc/gol_gen_plan.h gen_stream_max_k) runs the board shallower than 4 generations per pass, the same calls
are also timed with the debug option "rule_k" 4: the kernel above 256 registers, one wave per SIMD.  Each size runs as a
process of its own under its own time limit, and a size that fails ends the run.

Per row: the measured ratio beside the static one and the baseline's own spread (max / min of its repetitions).  No
ratio is fixed in advance.  The static ratio is counted, not tuned:
  VALU     per word and generation, 12 + 4 / M + 2 per set rule bit plus gen_decay's instructions
           per word (DECAY_VALU: the VALU instructions of gol_gen_stream<4, M, P, false> less those of <2, M, P, false>,
           per level and word, less the same difference of gol_rule_stream; hipcc -O3 --offload-arch=gfx950), times the
           recomputed-row factor (S + 2 K) / S of the plan at the depth that ran, over the baseline's 12 + 4 / M + 2 per
           bit times its own factor at K = 4
  traffic  1 + P planes loaded and stored per row against 1: reported beside it; the pass is latency-bound (4.12), so
           the static ratio is the VALU one

    python tools/board_generations_bench.py [--out profiles/board_generations/board_generations_bench.json] [--reps 7]
    python tools/board_generations_bench.py --size 4096      (one size, in this process; merges into --out)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((4096, 1000, 240), (16384, 256, 300), (65536, 64, 420))  # (size, generations, time limit s)
RULE, NSTATES = "B2/S345", (3, 4, 8)
STORED, TARGET_WAVES = 62, 8192  # gol_rule_plan.h; 32 waves on each of the MI355X's 256 CUs
PLANES = {3: 1, 4: 2, 8: 3}
# gen_decay's VALU instructions per word and generation by layout M and planes P (see above)
DECAY_VALU = {1: (1.33, 9.33, 16.0), 2: (3.67, 13.08, 18.08), 4: (3.67, 13.17, 18.17)}
# .vgpr_count of gol_gen_stream<K, M, P, BOUNDED>, [bounded, torus]; no kernel has scratch
KERNEL = {"gen_stream_vgprs": {
    "K4": {"M1": {"P1": [83, 65], "P2": [107, 83], "P3": [128, 110]},
           "M2": {"P1": [130, 102], "P2": [174, 134], "P3": [204, 176]},
           "M4": {"P1": [226, 202], "P2": [306, 272], "P3": [356, 308]}},
    "K2": {"M1": {"P1": [63, 49], "P2": [82, 63], "P3": [102, 80]},
           "M2": {"P1": [92, 69], "P2": [124, 89], "P3": [153, 128]},
           "M4": {"P1": [152, 131], "P2": [206, 171], "P3": [248, 203]}},
    "K1": {"M1": {"P1": [55, 41], "P2": [70, 54], "P3": [90, 68]},
           "M2": {"P1": [78, 55], "P2": [100, 69], "P3": [129, 106]},
           "M4": {"P1": [124, 103], "P2": [162, 131], "P3": [203, 159]}}},
    "note": "[bounded, torus]; scratch 0 everywhere; gol_step runs the deepest K with <= 256 (csrc/gol_gen_plan.h)"}


def max_k(ilv, planes):  # csrc/gol_gen_plan.h gen_stream_max_k
    return 4 if ilv < 4 or planes == 1 else 2


def factor(size, ilv, k):
    nstrips = -(-(size // (32 * ilv)) // STORED)
    seg = max(-(-size // max(TARGET_WAVES // nstrips, 1)), 2 * k)
    return seg, (seg + 2 * k) / seg


def static_ratio(size, ilv, nbits, planes, k):
    base = 12 + 4 / ilv + 2 * nbits
    new = base + DECAY_VALU[ilv][planes - 1]
    seg, f = factor(size, ilv, k)
    _, f4 = factor(size, ilv, 4)
    return {"new_valu_per_word_generation": round(new, 2), "baseline_valu_per_word_generation": round(base, 2),
            "depth": k, "segment_rows": seg, "recompute": round(f, 4), "baseline_recompute": round(f4, 4),
            "traffic_ratio": 1 + planes, "static_ratio": round(new * f / (base * f4), 4)}


def stats(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2), "max_us": round(max(us), 2)}


def one_size(size, gens, reps):
    from gameoflifewithactors_amd import Board, _lib

    birth, survive = _lib.rule_parse(RULE)
    nbits = bin(birth).count("1") + bin(survive).count("1")
    rows = {}
    with Board(size, size) as b:
        b.seed_splitmix(0x5EED)
        info = b.info()
        for nstates in NSTATES:
            planes = PLANES[nstates]
            table_k = max_k(info["ilv"], planes)
            for k in sorted({table_k, 4}):
                def measured():
                    b.set_rule((birth, survive, nstates)).set_option("rule_k", 0 if k == table_k else k)
                    us = b.step_timed(gens)
                    b.set_option("rule_k", 0)
                    return us, b.get_option("last_pass")

                def baseline():
                    return b.set_rule((birth, survive, 2)).step_timed(gens), b.get_option("last_pass")

                measured()
                baseline()
                got, base = [], []
                for _ in range(reps):
                    us, new_pass = measured()
                    got.append(us)
                    us, base_pass = baseline()
                    base.append(us)
                st = static_ratio(size, info["ilv"], nbits, planes, k)
                name = f"{RULE}/C{nstates}" + ("" if k == table_k else f" (rule_k {k})")
                rows[name] = dict(
                    st, nstates=nstates, planes=planes, table_depth=table_k, measured=stats(got),
                    baseline_two_states=stats(base), last_pass=new_pass, baseline_last_pass=base_pass,
                    us_per_generation=round(statistics.median(got) / gens, 4),
                    baseline_us_per_generation=round(statistics.median(base) / gens, 4),
                    ratio=round(statistics.median(got) / statistics.median(base), 4),
                    baseline_spread=round(max(base) / min(base), 4))
                print(size, name, json.dumps(rows[name]), flush=True)
    return {"generations_per_call": gens, "ilv": info["ilv"], "rows": rows}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "board_generations", "board_generations_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=0)
    a = ap.parse_args()
    if a.size:
        gens = {s: g for s, g, _ in SIZES}[a.size]
        result = json.load(open(a.out)) if os.path.exists(a.out) else {}
        result.setdefault("sizes", {})[str(a.size)] = one_size(a.size, gens, a.reps)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"boundary": "torus", "init": "gol_seed_splitmix(0x5EED)", "rule": RULE, "reps": a.reps,
                   "timing": "HIP events on the board's stream (gol_step_timed), one warm-up call of each kind first, a "
                             "baseline call (the same B/S at two states: gol_rule_stream) after every measured call",
                   "kernel": KERNEL, "decay_valu_per_word": DECAY_VALU, "sizes": {}}, f, indent=1)
    for size, _, limit in SIZES:  # a process and a time limit per size; the first that fails ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--size",
                             str(size), "--out", a.out, "--reps", str(a.reps)]).returncode
        if rc != 0:
            print(f"size {size}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
