#!/usr/bin/env python
"""Device time of a single board under a life-like rule (gol_set_rule: the single-wave pass with the rule table at
100^2, the rule-generic streaming pass csrc/gol_rule_step.hip above) beside the same board under B3/S23 on its default
pass -- the parent's unchanged kernels (profiles/board_rules/README.md).

Torus, gol_seed_splitmix, HIP events on the board's stream (gol_step_timed), one warm-up call of each kind and --reps
repetitions, one baseline call after every measured call.  Measured: B3/S23 forced through the rule family (debug option
"rule_table"), B36/S23, B3678/S34678.  A step's time does not depend on the cells, so every call steps whatever the
previous one left.  Each size runs as a process of its own under its own time limit, and a size that fails ends the run.

Per row: the measured ratio, the static ratio and the baseline's own spread (max / min of its repetitions), and "within"
or "above" the product of the last two.  The static ratio is counted, not tuned:
  rule stream   VALU instructions per word and generation of the loop of gol_rule_stream<4, M, false> in the disassembly
                (hipcc -O3 --offload-arch=gfx950): 12 per word (2 row sum, 9 planes and qualifiers, 1 cleared
                accumulator) + 4 per block of M words (2 DPP moves, 2 v_alignbit) + 2 per word and set rule bit, times
                the recomputed-row factor (S + 2 K) / S of the plan (gol_rule_plan.h, K = 4), over the baseline pass's
                published count per word and generation (BASELINE_VALU below)
  single wave   121 + 16 per set bit against 96 VALU per generation (the batch's kernel body)

    python tools/board_rules_bench.py [--out profiles/board_rules/board_rules_bench.json] [--reps 7]
    python tools/board_rules_bench.py --size 4096      (one size, in this process; merges into --out)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((100, 1000, 120), (4096, 1000, 240), (16384, 256, 300), (65536, 64, 420))  # (size, generations, time limit s)
MEASURED = (("B3/S23", True), ("B36/S23", False), ("B3678/S34678", False))  # (rule, forced through the rule family)
K, STORED, TARGET_WAVES = 4, 62, 8192  # gol_rule_plan.h, gol_rule_step.hip; 32 waves on each of the MI355X's 256 CUs
# the baseline pass's published VALU per word and generation, recomputed rows included: the cooperative pass 38.6 per
# wave of 2 words, the streaming pass 11.93 measured (0 item 3), the level-pipelined pass 686.75M
# per launch of 32 generations of 2^27 words over 64 lanes (4.7)
BASELINE_VALU = {4096: ("cooperative", 19.3), 16384: ("streaming", 11.93), 65536: ("level-pipelined", 10.23)}
KERNEL = {"rule_stream_vgprs": {"K8_M1": [73, 93], "K8_M2": [136, 160], "K8_M4": [268, 293], "K4_M4": [150, 160]},
          "note": "[torus, bounded]; scratch 0 everywhere; > 256 = AGPRs as the allocator's overflow"}


def bits(rule, lib):
    birth, survive = lib.rule_parse(rule)
    return bin(birth).count("1") + bin(survive).count("1")


def static_ratio(size, ilv, nbits):
    if size == 100:
        return {"new_valu_per_generation": 121 + 16 * nbits, "baseline_valu_per_generation": 96, "recompute": 1.0,
                "static_ratio": round((121 + 16 * nbits) / 96, 4)}
    nblocks = size // (32 * ilv)
    nstrips = -(-nblocks // STORED)
    seg = max(-(-size // max(TARGET_WAVES // nstrips, 1)), 2 * K)
    new = 12 + 4 / ilv + 2 * nbits
    factor = (seg + 2 * K) / seg
    name, base = BASELINE_VALU[size]
    return {"new_valu_per_word_generation": round(new, 2), "segment_rows": seg, "recompute": round(factor, 4),
            "baseline_pass": name, "baseline_valu_per_word_generation": base,
            "static_ratio": round(new * factor / base, 4)}


def stats(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2), "max_us": round(max(us), 2)}


def one_size(size, gens, reps):
    from gameoflifewithactors_amd import Board, _lib

    rows = {}
    with Board(size, size) as b:
        b.seed_splitmix(0x5EED)
        info = b.info()
        for rule, forced in MEASURED:
            def measured():
                b.set_option("rule_table", int(forced))
                us = b.set_rule(rule).step_timed(gens)
                b.set_option("rule_table", 0)
                return us, b.get_option("last_pass")

            def baseline():
                return b.set_rule("B3/S23").step_timed(gens), b.get_option("last_pass")

            measured()
            baseline()
            got, base = [], []
            for _ in range(reps):
                us, new_pass = measured()
                got.append(us)
                us, base_pass = baseline()
                base.append(us)
            st = static_ratio(size, info["ilv"], bits(rule, _lib))
            spread = max(base) / min(base)
            ratio = statistics.median(got) / statistics.median(base)
            margin = st["static_ratio"] * spread
            rows[rule + (" (rule_table)" if forced else "")] = dict(
                st, measured=stats(got), baseline_b3s23=stats(base), last_pass=new_pass, baseline_last_pass=base_pass,
                us_per_generation=round(statistics.median(got) / gens, 4),
                baseline_us_per_generation=round(statistics.median(base) / gens, 4), ratio=round(ratio, 4),
                baseline_spread=round(spread, 4), margin=round(margin, 4),
                verdict="within" if ratio <= margin else "above", excess=round(max(ratio / margin - 1, 0.0), 4))
            print(size, rule, json.dumps(rows[rule + (" (rule_table)" if forced else "")]), flush=True)
    return {"generations_per_call": gens, "ilv": info["ilv"], "tblock_k": info["tblock_k"], "rows": rows}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "board_rules", "board_rules_bench.json"))
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
        json.dump({"boundary": "torus", "init": "gol_seed_splitmix(0x5EED)", "reps": a.reps,
                   "timing": "HIP events on the board's stream (gol_step_timed), one warm-up call of each kind first, a "
                             "baseline call (B3/S23, default pass) after every measured call",
                   "kernel": KERNEL, "sizes": {}}, f, indent=1)
    for size, _, limit in SIZES:  # a process and a time limit per size; the first that fails ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--size",
                             str(size), "--out", a.out, "--reps", str(a.reps)]).returncode
        if rc != 0:
            print(f"size {size}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
