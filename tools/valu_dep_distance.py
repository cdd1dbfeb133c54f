"""Dependent distance of the level-pipelined pass's rule instructions, from a device listing (no GPU).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -x hip --cuda-device-only -S -I include -I <csrc> <csrc>/gol_pipe.hip -o pipe.s
    python tools/valu_dep_distance.py pipe.s

For every gol_pipe_step kernel of the listing and each of its three trip loops (fill, full trips, last trip: the
loops that hold v_bitop3_b32, in program order) it prints the v_bitop3_b32 / v_alignbit_b32 / v_mov_b32_dpp counts and,
for v_bitop3_b32 and for v_alignbit_b32, the histogram of the distance, counted in VALU instructions, back to the
nearest earlier VALU instruction that wrote one of the instruction's sources (1: the instruction right before it).
The histogram is given per basic block that holds such instructions (the levels are one block; a stage branch's own
block shows up beside it) and for the loop as a whole.  A source written by an LDS or buffer read, or before the
block began (loop-carried, or from another stage branch), counts as far: it falls in the last column with the
distances of 8 and more.  It also lists whatever else stands between a block's first and last rule instruction (the
s_nop of level_align apart): a 4-byte instruction there flips the address parity of every level after it (DESIGN.md
4.7), and the kernel's register envelope from the listing's own summary.  Why the distance matters: DESIGN.md 4.7
"dependent distance" (at 4 waves per SIMD an instruction 2-4 behind its producer issues 4-12 % slower than one 8 or
more behind).
"""
from __future__ import annotations

import collections
import re
import sys

FAR = 8  # the last column: 8 or more, or no VALU producer in the block
KINDS = ("v_bitop3_b32", "v_alignbit_b32")
RULE = KINDS + ("v_mov_b32_dpp",)
LOOPS = ("fill", "full trips", "last trip")

_REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def _regs(operand: str) -> list[int]:
    out = []
    for m in _REG.finditer(operand):
        if m.group(1) is not None:
            out.append(int(m.group(1)))
        else:
            out.extend(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def _operands(rest: str) -> list[str]:
    rest = rest.split(";")[0]
    return [o.strip() for o in rest.split(",")] if rest.strip() else []


def kernels(text: str) -> dict[str, list[str]]:
    """{mangled name: its lines} of every gol_pipe_step kernel in the listing"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\S*gol_pipe_step\S*):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.strip().startswith(".Lfunc_end"):
            cur = None
            continue
        out[cur].append(line)
    return out


def envelopes(text: str) -> dict[str, dict]:
    """{mangled name: {"vgprs", "scratch", "occupancy"}} from the summary the compiler writes behind each kernel"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\S*gol_pipe_step\S*):", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", line)
        if m and cur is not None and m.group(1) not in cur:
            cur[m.group(1)] = int(m.group(2))
    return {k: {"vgprs": v.get("NumVgprs"), "scratch": v.get("ScratchSize"), "occupancy": v.get("Occupancy")}
            for k, v in out.items()}


def short_name(mangled: str) -> str:
    m = re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])E", mangled)
    if not m:
        return mangled
    d, s, p, wrap, bnd = (int(x) for x in m.groups())
    kind = "torus" if wrap else ("bounded" if bnd else "ghost-row")
    return f"K={d * s} {kind} (gol_pipe_step<{d}, {s}, {p}, {bool(wrap)}, {bool(bnd)}>)".replace("True", "true").replace("False", "false")


def trip_loops(lines: list[str]) -> list[list[str]]:
    """The kernel's depth-1 loops that hold v_bitop3_b32, in program order, each as its lines (header to last member)"""
    spans = {}  # header label -> [first line, last line]
    order = []
    for i, line in enumerate(lines):
        m = re.match(r"^\.(LBB\d+_\d+):\s*;\s*=>This Inner Loop Header: Depth=1", line) or \
            re.match(r"^\.(LBB\d+_\d+):\s*;\s*=>This Loop Header: Depth=1", line)
        if m:
            spans[m.group(1)] = [i, i]
            order.append(m.group(1))
            continue
        m = re.search(r";\s+in Loop: Header=(BB\d+_\d+) Depth=1", line)
        if m and "L" + m.group(1) in spans:
            spans["L" + m.group(1)][1] = i
    loops = []
    for h in order:
        a, b = spans[h]
        # a block runs on to the next label: take the lines up to the one before the label after the last member
        e = b + 1
        while e < len(lines) and not re.match(r"^\.LBB\d+_\d+:", lines[e]) and not lines[e].startswith("; %bb."):
            e += 1
        body = lines[a:e]
        if any(l.split() and l.split()[0] == "v_bitop3_b32" for l in body):
            loops.append(body)
    return loops


def analyse_loop(body: list[str]) -> dict:
    """counts and, per block and kind, {distance 1..FAR: instructions}"""
    counts = collections.Counter()
    inside = collections.Counter()  # other instructions between a block's first and last rule instruction
    pending, seen_rule, in_rept = [], False, False
    blocks = []  # (label, {kind: Counter})
    label, hist = "head", {k: collections.Counter() for k in KINDS}
    writer = {}  # VGPR -> index of the VALU instruction that wrote it, in this block
    n = 0

    def close():
        nonlocal hist, writer, pending, seen_rule
        pending, seen_rule = [], False
        if any(hist[k] for k in KINDS):
            blocks.append((label, hist))
        hist = {k: collections.Counter() for k in KINDS}
        writer = {}

    for line in body:
        s = line.strip()
        m = re.match(r"^\.?(LBB\d+_\d+|\d+):", s)
        if m or s.startswith("; %bb."):
            close()
            label = m.group(1) if m else s.split()[1].rstrip(":")
            continue
        if s.startswith((".rept", ".endr")):
            in_rept = s.startswith(".rept")
            continue
        if not s or s.startswith((";", ".", "//")) or in_rept:
            continue
        parts = s.split(None, 1)
        op, ops = parts[0], _operands(parts[1] if len(parts) > 1 else "")
        if op in RULE:
            inside.update(pending)
            pending, seen_rule = [], True
        elif seen_rule:
            pending.append(op)
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm")):
            close()
            label = label + "+"
            continue
        if op.startswith("v_"):
            n += 1
            if op in RULE:
                counts[op] += 1
            writes_vgpr = not op.startswith(("v_cmp", "v_readfirstlane", "v_readlane"))
            srcs = ops[1:] if writes_vgpr else ops
            if op in KINDS:
                d = [n - writer[r] for o in srcs for r in _regs(o) if r in writer]
                dist = min(d) if d else FAR
                hist[op][min(dist, FAR)] += 1
            if writes_vgpr and ops:
                for r in _regs(ops[0]):
                    writer[r] = n
        elif op.startswith(("ds_read", "ds_load", "buffer_load", "global_load", "flat_load", "scratch_load")) and ops:
            for r in _regs(ops[0]):
                writer.pop(r, None)  # from memory: far
    close()
    total = {k: collections.Counter() for k in KINDS}
    for _, h in blocks:
        for k in KINDS:
            total[k].update(h[k])
    return {"counts": dict(counts), "blocks": blocks, "total": total, "inside": dict(inside)}


def analyse(text: str) -> dict:
    """{kernel short name: {"envelope": envelopes()' entry, "loops": {loop name: analyse_loop()}}}; a kernel whose fill
    the compiler unrolled has the last two loops only"""
    out, env = {}, envelopes(text)
    for name, lines in kernels(text).items():
        loops = trip_loops(lines)
        names = LOOPS[len(LOOPS) - len(loops):] if len(loops) <= len(LOOPS) else [f"loop {i}" for i in range(len(loops))]
        out[short_name(name)] = {"envelope": env.get(name, {}), "loops": {names[i]: analyse_loop(b) for i, b in enumerate(loops)}}
    return out


def share(hist, dists) -> float:
    n = sum(hist.values())
    return sum(hist[d] for d in dists) / n if n else 0.0


def _row(label: str, hist) -> str:
    n = sum(hist.values())
    cells = " ".join(f"{hist[d]:5d}" for d in range(1, FAR + 1))
    pct = " ".join(f"{100.0 * hist[d] / n:5.1f}" for d in range(1, FAR + 1)) if n else ""
    return f"    {label:<22s} n={n:4d} | {cells} | % {pct}"


def render(res: dict) -> str:
    out = []
    head = " ".join(f"{d:5d}" for d in range(1, FAR)) + "    8+"
    for kname, k in res.items():
        e = k["envelope"]
        out.append(f"{kname}: {e.get('vgprs')} VGPRs, scratch {e.get('scratch')}, occupancy {e.get('occupancy')}")
        for lname, a in k["loops"].items():
            c = a["counts"]
            out.append(f"  {lname}: v_bitop3_b32 {c.get('v_bitop3_b32', 0)}, v_alignbit_b32 {c.get('v_alignbit_b32', 0)}, "
                       f"v_mov_b32_dpp {c.get('v_mov_b32_dpp', 0)}")
            for k in KINDS:
                out.append(f"   {k}: distance to the nearest VALU producer   {head}")
                for label, h in a["blocks"]:
                    if h[k]:
                        out.append(_row("block " + label, h[k]))
                out.append(_row("loop", a["total"][k]))
            other = ", ".join(f"{n} {op}" for op, n in sorted(a["inside"].items())) or "none"
            out.append(f"   other instructions between a block's first and last rule instruction: {other}")
            out.append(f"   v_bitop3_b32 at distance 2 or 3: {100.0 * share(a['total']['v_bitop3_b32'], (2, 3)):.1f} %")
    return "\n".join(out) + "\n"


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    sys.stdout.write(render(analyse(open(sys.argv[1]).read())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
