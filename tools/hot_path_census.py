#!/usr/bin/env python3
"""hot_path_census.py LISTING KERNEL-REGEX: what does every basic block of a kernel issue?

LISTING is device assembly of a sweep unit, e.g. the one-wave backward sweeps with the Makefile's flags:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Wno-unused-function -mllvm -amdgpu-mfma-vgpr-form -DKP_FUSED_PART=1 \\
          -S --cuda-device-only trajoptkp_amd/csrc/fused_mfma.hip -o part1.s

KERNEL-REGEX is searched in the demangled name and in the symbol of every function of the listing (kernels and the out-of-line device
functions they call); every match is reported.  Per basic block -- `.LBBf_n:` and the fall-through blocks `; %bb.n:` -- with the loop
depth the compiler wrote beside it, the counts of

    mfma    matrix instructions                         lds     ds_*
    fp      FP VALU (v_*_f64 / _f32 / _f16 / _bf16)     mem     buffer_* / global_* / flat_* / scratch_*
    mov     v_mov*                                      nop     CYCLES of s_nop (s_nop n idles n + 1)
    cnd     v_cndmask*                                  salu    every other s_* (waits and branches included)
    acc     v_accvgpr_read / _write
    valu    every other v_*

and below the table the register summary (NumVgprs, NumAgprs, ScratchSize, Occupancy).  Instruction classes are counted, nothing
else: which blocks a step runs through is read off the listing by hand (profiles/backward_fast_path_census.txt names them)."""
import re
import subprocess
import sys

CLASSES = ("mfma", "fp", "mov", "cnd", "acc", "valu", "lds", "mem", "nop", "salu")


def classify(op, operands):
    """(class, count) of one instruction, or None for what is no instruction of the wave (directives never get here)"""
    if op.startswith(("v_mfma", "v_smfmac")): return "mfma", 1
    if op.startswith("v_accvgpr"): return "acc", 1
    if op.startswith("v_mov"): return "mov", 1
    if op.startswith("v_cndmask"): return "cnd", 1
    if op.startswith("v_"):
        return ("fp" if re.search(r"_(f64|f32|f16|bf16)(_|$)", op) else "valu"), 1
    if op.startswith("ds_"): return "lds", 1
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")): return "mem", 1
    if op == "s_nop":
        return "nop", int(operands.split()[0], 0) + 1
    if op.startswith("s_"): return "salu", 1
    return None


def functions(lines):
    """[(symbol, first line, line behind the last)] of every function of the listing"""
    out, cur = [], None
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m and cur is None: cur = (m.group(1), i)
        elif l.startswith(".Lfunc_end") and cur: out.append((cur[0], cur[1], i)); cur = None
    return out


def census(lines):
    """[(label, depth, {class: count})] of the blocks of one function's lines"""
    blocks = []
    cur = ["entry", 0, dict.fromkeys(CLASSES, 0)]
    for l in lines:
        m = re.match(r"^(?:(\.LBB\d+_\d+):|; (%bb\.\d+):)", l)
        if m:
            blocks.append(cur)
            cur = [m.group(1) or m.group(2), 0, dict.fromkeys(CLASSES, 0)]
        d = re.search(r"Depth=(\d+)", l)
        if d and l.lstrip().startswith((";", ".LBB")): cur[1] = max(cur[1], int(d.group(1)))
        code = l.split(";")[0].strip()
        if not code or code.startswith(".") or code.endswith(":"): continue
        op, _, operands = code.partition(" ")
        c = classify(op, operands)
        if c: cur[2][c[0]] += c[1]
    blocks.append(cur)
    return [b for b in blocks if any(b[2].values())]


def main():
    if len(sys.argv) != 3: sys.exit(__doc__)
    lines = open(sys.argv[1]).read().split("\n")
    funcs = functions(lines)
    names = subprocess.run(["c++filt"], input="\n".join(f[0] for f in funcs), capture_output=True, text=True, check=True).stdout.splitlines()
    pat, found = re.compile(sys.argv[2]), 0
    for (sym, lo, hi), name in zip(funcs, names):
        if not (pat.search(name) or pat.search(sym)): continue
        found += 1
        print(name.rsplit("(", 1)[0])
        print("  %-12s %5s " % ("block", "depth") + " ".join("%5s" % c for c in CLASSES))
        total = dict.fromkeys(CLASSES, 0)
        for label, depth, cnt in census(lines[lo:hi]):
            print("  %-12s %5d " % (label, depth) + " ".join("%5d" % cnt[c] for c in CLASSES))
            for c in CLASSES: total[c] += cnt[c]
        print("  %-12s %5s " % ("all blocks", "") + " ".join("%5d" % total[c] for c in CLASSES))
        summary = []
        for l in lines[hi:hi + 400]:
            m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", l)
            if m: summary.append("%s %s" % m.groups())
            if l.startswith("; Occupancy") or re.match(r"^_Z\w+:", l): break
        print("  registers: " + ", ".join(summary) + "\n")
    if not found: sys.exit("no function of %s matches %r" % (sys.argv[1], sys.argv[2]))


if __name__ == "__main__":
    main()
