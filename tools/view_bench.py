#!/usr/bin/env python
"""Device time of the board view (gol_strip_view_counts) beside the full-board reduction that reads the same bytes.

A 65536^2 torus in the engine's default layout, one wrap_rows strip through HipEngine, seeded splitmix 0x5EED and
advanced 160 generations.  Four views -- the whole board at s = 64, 128 and 4096, and a 1920 x 1080 window at s = 8 --
are timed with torch events on the strip's stream, 5 warm-up and 20 timed repetitions each, every repetition followed
IN THE SAME PROCESS by one of gol_strip_population on the same buffer: the yardstick, since a whole-board view reads
exactly the bytes the population does.  Also the end-to-end host time of Board.render_view for the s = 64 frame.

    python tools/view_bench.py [--out profiles/view/view_bench.json] [--size 65536] [--reps 20] [--warmup 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gameoflifewithactors_amd import Board, _lib  # noqa: E402
from gameoflifewithactors_amd.strips import StripRunner  # noqa: E402

PEAK_BPS = 8e12         # the HBM peak the README's fractions use
PASS_US = (962.0, 990.0)  # one K = 32 pass of the 65536^2 board (README)


def stats(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2), "max_us": round(max(us), 2)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view", "view_bench.json"))
    ap.add_argument("--size", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    n, dev = a.size, torch.device("cuda", 0)
    views = {
        "whole_s64": (0, 0, 64, n // 64, n // 64),
        "whole_s128": (0, 0, 128, n // 128, n // 128),
        "whole_s4096": (0, 0, 4096, n // 4096, n // 4096),
        "window_1920x1080_s8": (n // 2 - 960 * 8, n // 2 - 540 * 8, 8, 1920, 1080),
    }
    result = {"board": [n, n], "boundary": "torus", "seed": 0x5EED, "generations": 160, "reps": a.reps,
              "warmup": a.warmup, "peak_bytes_per_s": PEAK_BPS, "device": torch.cuda.get_device_name(0), "cases": {}}
    with StripRunner(n, n, _lib.TORUS, 32, device=dev) as r:
        r.seed_splitmix(0x5EED)
        r.step(160)
        eng, geom, buf, stream = r.engine, r.geom, r.bufs[r.cur], r.compute_stream
        result["ilv"], result["pitch_words"] = geom.ilv, geom.pitch
        pop_acc = eng.reduce(geom, buf, "population", stream)
        stream.synchronize()
        want_pop = int(pop_acc.cpu()[0])
        result["population"] = want_pop
        for name, view in views.items():
            x, y, s, out_w, out_h = view
            with torch.cuda.stream(stream):
                counts = torch.zeros(out_w * out_h, dtype=torch.int32, device=dev)
                acc = torch.zeros(1, dtype=torch.int64, device=dev)
            strip = geom.strip()
            v = _lib.View(*view)
            def run_view():
                _lib.check(eng.lib.gol_strip_view_counts(ctypes.byref(strip), buf.data_ptr(), ctypes.byref(v),
                                                         counts.data_ptr(), stream.cuda_stream), "view")

            def run_pop():
                _lib.check(eng.lib.gol_strip_population(ctypes.byref(strip), buf.data_ptr(), acc.data_ptr(),
                                                        stream.cuda_stream), "population")

            t_view, t_pop = [], []
            for rep in range(a.warmup + a.reps):
                for fn, sink in ((run_view, t_view), (run_pop, t_pop)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= a.warmup:
                        sink.append(e0.elapsed_time(e1) * 1e3)
            # the counts were added warmup + reps times: a whole-board view then holds that multiple of the population
            total = int(counts.cpu().to(torch.int64).sum())
            whole = s * out_w == n and s * out_h == n
            if whole and total != (a.warmup + a.reps) * want_pop:
                print(f"{name}: counts sum {total} != {(a.warmup + a.reps)} x population {want_pop}", file=sys.stderr)
                return 1
            nbytes = (s * out_w) * (s * out_h) // 8
            med = statistics.median(t_view)
            case = {"view": list(view), "view_us": stats(t_view), "population_us": stats(t_pop),
                    "algorithmic_bytes": nbytes, "gb_per_s": round(nbytes / med / 1e3, 1),
                    "fraction_of_peak": round(nbytes / (med * 1e-6) / PEAK_BPS, 4),
                    "median_within_population_spread": bool(min(t_pop) <= med <= max(t_pop)) if whole else None,
                    "median_below_population_max": bool(med <= max(t_pop)) if whole else None}
            if name == "whole_s64":
                case["fraction_of_k32_pass"] = [round(med / PASS_US[1], 4), round(med / PASS_US[0], 4)]
            result["cases"][name] = case
            print(name, json.dumps(case), flush=True)
    # end to end through the board handle: kernel, tone map, copy of 1024^2 bytes, synchronisation
    with Board(n, n) as b:
        b.seed_splitmix(0x5EED)
        b.step(160)
        b.synchronize()
        x, y, s, out_w, out_h = views["whole_s64"]
        host = []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            b.render_view(x, y, s, out_w, out_h, _lib.VIEW_DENSITY, 255)
            if rep >= a.warmup:
                host.append((time.perf_counter() - t0) * 1e6)
        result["render_view_s64_host_us"] = stats(host)
        print("render_view_s64_host_us", json.dumps(result["render_view_s64_host_us"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
