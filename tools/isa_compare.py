#!/usr/bin/env python
"""Compare every kernel's instruction stream between two trees of csrc/ (the parent's and this one's): cross-compile each
.hip file of both to gfx950 assembly, renumber the labels of each kernel in order of appearance, and compare kernel by
kernel.  Template arguments that only a later revision has (an empty trailing parameter pack) are dropped from the name
before matching, so a kernel that gained an empty pack still meets its parent.  --rename OLD=NEW (a regular expression
and its replacement, on the demangled name; may be given several times) gives a parent kernel the name it has in this
tree, where a kernel was renamed or gained a template argument: it is then compared and counted as renamed, not as
missing and new.

A file argument PARENT.hip=THIS.hip[+THIS2.hip ...] compares the parent's kernels of PARENT.hip with the union of the
kernels of this tree's THIS.hip, THIS2.hip, ...: for kernels that moved between files.

    python tools/isa_compare.py [--rename OLD=NEW ...] <parent csrc dir> <this csrc dir> file.hip [file.hip ...]
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assembly(csrc, name, out):
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(csrc))), "include")
    if not os.path.isdir(inc):
        inc = os.path.join(ROOT, "include")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only",
                    "-S", "-I", inc, "-I", csrc, os.path.join(csrc, name), "-o", out], check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read()


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(text):
    """{demangled name: [instruction lines, labels renumbered]} of every .amdhsa_kernel of the file."""
    wanted = set(re.findall(r"\.amdhsa_kernel\s+(\S+)", text))
    body, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(\S+):\s*(;.*)?$", line)
        if m and m.group(1) in wanted:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if not s or (s.startswith(".") and not re.match(r"^\.LBB\d+_\d+:", s)):
            continue
        body[cur].append(s)
    names = demangle(sorted(body))
    out = {}
    for sym, lines in body.items():
        seen = {}
        def ren(m):
            return seen.setdefault(m.group(0), f".L{len(seen)}")
        out[re.sub(r",\s*>", ">", re.sub(r"\s+", " ", names[sym]))] = [re.sub(r"\.LBB\d+_\d+", ren, l) for l in lines]
    return out


def renamed(name, renames):
    """The name a parent kernel has in this tree: every OLD=NEW applied in order (re.sub on the demangled name)."""
    for old, new in renames:
        name = re.sub(old, new, name)
    return name


def main():
    args, renames = sys.argv[1:], []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    parent, this, files = args[0], args[1], args[2:]
    bad = 0
    with tempfile.TemporaryDirectory() as d:
        for f in files:
            left, _, right = f.partition("=")
            a = kernels(assembly(parent, left, os.path.join(d, "a.s")))
            b = {}
            for g in (right or left).split("+"):
                b.update(kernels(assembly(this, g, os.path.join(d, "b.s"))))
            was = {renamed(k, renames): k for k in a}  # this tree's name -> the parent's
            a = {renamed(k, renames): v for k, v in a.items()}
            moved = [k for k in a if was[k] != k and k in b]
            same = [k for k in a if k in b and a[k] == b[k]]
            diff = [k for k in a if k in b and a[k] != b[k]]
            gone = [k for k in a if k not in b]
            new = [k for k in b if k not in a]
            print(f"{f}: {len(a)} kernels in the parent, {len(same)} identical, {len(diff)} differ, {len(gone)} missing, "
                  f"{len(new)} new" + (f", {len(moved)} renamed" if renames else ""))
            for k in diff + gone:
                print("   ", "DIFFERS" if k in diff else "MISSING", was[k])
                if k in moved:
                    print("        renamed to", k)
            bad += len(diff) + len(gone)
    print("all parent kernels identical" if not bad else f"{bad} parent kernels differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
