#!/usr/bin/env python3
"""Instruction census of the MSM accumulate loops (no GPU needed).

Compiles csrc/msm.hip device-only to gfx950 assembly (the Makefile's flags) and
prints, for the main loop of every k_msm_accumulate* kernel, how many VALU
instructions it holds and how many of them are the two 64-bit mads, v_mov*,
v_cndmask*, plus s_nop, ds_* and global_load_lds*; then the kernel's NumVgprs,
ScratchSize and Occupancy.  The main loop is the backward branch spanning the
most mads.  Regions a forward s_cbranch_execz jumps over are listed by their
assembly lines: one holding more mads than any other and than the code around
them is the addition and is searched in turn; the others (the flush, the run
start, the exceptional cases) are taken off the "main path" row.

  accumulate_census.py [--asm FILE] [--tag NAME] [-D...]

--asm reads an assembly file instead of compiling; -D flags go to the compiler.
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
FLAGS = ["-std=c++17", "-O3", "--offload-arch=gfx950", "-fPIC", "-mllvm",
         "-pragma-unroll-threshold=100000", "--cuda-device-only", "-S"]
CLASSES = [
    ("valu", re.compile(r"^v_")),
    ("mad_u64", re.compile(r"^v_mad_u64_u32")),
    ("mad_i64", re.compile(r"^v_mad_i64_i32")),
    ("v_mov", re.compile(r"^v_mov")),
    ("v_cndmask", re.compile(r"^v_cndmask")),
    ("s_nop", re.compile(r"^s_nop")),
    ("ds", re.compile(r"^ds_")),
    ("load_lds", re.compile(r"^global_load_lds")),
]


def compile_asm(defs):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + FLAGS + defs + [os.path.join(PKG, "csrc", "msm.hip"), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)
    return out


def kernels(lines):
    """(name, first, last) line ranges of the k_msm_accumulate* functions"""
    out = []
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w*k_msm_accumulate\w*):", ln)
        if m:
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            out.append((m.group(1), i, j))
    return out


def count(ops):
    c = {k: 0 for k, _ in CLASSES}
    for op in ops:
        for k, rx in CLASSES:
            if rx.match(op):
                c[k] += 1
    return c


def mads(c):
    return c["mad_u64"] + c["mad_i64"]


def census(lines, first, last):
    body = lines[first:last]
    label = {}
    ops = []  # (index in body, mnemonic, operand text)
    for i, ln in enumerate(body):
        s = ln.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            label[m.group(1)] = i
        elif s and not s.startswith((";", ".")):
            parts = s.split(None, 1)
            ops.append((i, parts[0], parts[1] if len(parts) > 1 else ""))
    # the main loop: the backward branch whose span holds the most mads
    best = None
    for i, op, arg in ops:
        if op.startswith(("s_cbranch", "s_branch")):
            t = label.get(arg.split()[0])
            if t is not None and t < i:
                n = mads(count(o for j, o, _ in ops if t <= j <= i))
                if best is None or n > best[0]:
                    best = (n, t, i)
    if best is None:
        return None
    _, lo, hi = best
    loop = [(j, o, a) for j, o, a in ops if lo <= j <= hi]
    total = count(o for _, o, _ in loop)
    main = dict(total)
    rows = []

    def walk(lo, hi, level_mads, depth):
        """forward execz-skipped regions of [lo, hi], outermost first.  The
        addition is where most mads of a level are: in its straight-line code,
        or in one region, which is then searched in turn; every other region
        (the flush, the run start, the exceptional cases) is off the main path."""
        found, end = [], -1
        for j, o, a in loop:
            if lo <= j <= hi and o == "s_cbranch_execz" and j > end:
                t = label.get(a.split()[0])
                if t is None or not j < t <= hi:
                    continue
                end = t
                found.append((j, t, count(o2 for j2, o2, _ in loop if j < j2 < t)))
        straight = level_mads - sum(mads(c) for _, _, c in found)
        top = max([mads(c) for _, _, c in found] + [straight])
        for j, t, c in found:
            rare = not (mads(c) == top and top > straight)
            rows.append((depth, j + first + 1, t + first + 1, c, rare))
            if rare:
                for k in main:
                    main[k] -= c[k]
            else:
                walk(j + 1, t - 1, mads(c), depth + 1)

    walk(lo, hi, mads(total), 0)
    return total, main, rows


def meta(lines, last):
    out = {}
    for ln in lines[last:last + 200]:
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", ln)
        if m and m.group(1) not in out:
            out[m.group(1)] = int(m.group(2))
    return out


def main(argv):
    asm, tag, defs = None, "", []
    it = iter(argv)
    for a in it:
        if a == "--asm":
            asm = next(it)
        elif a == "--tag":
            tag = next(it)
        elif a.startswith("-D"):
            defs.append(a)
        else:
            sys.exit(__doc__)
    path = asm or compile_asm(defs)
    with open(path) as f:
        lines = f.read().split("\n")
    if asm is None:
        os.unlink(path)
    keys = [k for k, _ in CLASSES]
    print(f"== accumulate census {tag} {' '.join(defs)}".rstrip())
    for name, first, last in kernels(lines):
        r = census(lines, first, last)
        m = meta(lines, last)
        print(f"{name}: NumVgprs {m.get('NumVgprs')} ScratchSize {m.get('ScratchSize')} "
              f"Occupancy {m.get('Occupancy')}")
        if r is None:
            print("  no loop found")
            continue
        total, mainp, rows = r
        print("  %-26s" % "" + " ".join("%9s" % k for k in keys))
        print("  %-26s" % "loop body" + " ".join("%9d" % total[k] for k in keys))
        print("  %-26s" % "main path" + " ".join("%9d" % mainp[k] for k in keys))
        for d, a, b, c, rare in rows:
            what = "  " * d + ("skipped" if rare else "addition")
            print("  %-26s" % f" {what} {a}-{b}" + " ".join("%9d" % c[k] for k in keys))
        other = mainp["valu"] - mads(mainp)
        print(f"  main path: {mads(mainp)} mads + {other} other VALU "
              f"({mainp['v_mov']} v_mov, {mainp['v_cndmask']} v_cndmask), {mainp['s_nop']} s_nop")


if __name__ == "__main__":
    main(sys.argv[1:])
