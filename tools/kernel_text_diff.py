#!/usr/bin/env python3
"""kernel_text_diff.py OLD_TREE NEW_TREE [--keep DIR]: are the sweep kernels of two trees the same instructions?

Compiles the sweep units of both trees to device assembly with the flags their own Makefile gives them (make -n; -c becomes
-S --cuda-device-only), pairs the kernels by name -- OLD_TREE's name suffixes _excl / _retry / _listed read as the trailing template
flags EXCL / GATED / LISTED, defaults filled in; a name that has its flags maps to itself -- and compares, per
pair, the text from the kernel's label to its .end_amdhsa_kernel: every instruction and every .amdhsa_* directive.  Dropped before
the comparison: comments, the numbering of local labels, the spelling of the kernel's own symbol, and .amdhsa_kernarg_size (a trailing
argument nobody reads costs kernarg bytes and nothing else).  Prints per unit: kernels compared, equal, different; the names that found
no partner and the first differing line of each pair that differs.  --keep DIR: leave the .s files in DIR/old, DIR/new and use the
ones already there.  Exit status 1 if anything differs."""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

UNITS = ("riccati_mfma", "forward_mfma", "generic", "tiled_mfma", "tiled_wide", "fused_mfma_1", "fused_mfma_2", "fused_mfma_3")
# the kernels that had name suffixes and have trailing flags (generic.hip keeps its suffixes): name -> (template arguments in all, has
# EXCL in front of GATED | LISTED)
FLAGGED = {"k_backward_mfma": (5, True), "k_backward_fused": (8, True), "k_backward_fusedph": (7, False),
           "k_forward_mfma": (4, True), "k_forward_fused": (8, True), "k_forward_fused_scu": (5, False), "k_forward_fused_sc3": (5, False)}


def flag_name(name):
    """k_backward_mfma_excl_retry<14, 7> -> k_backward_mfma<14, 7, 0, true, true>; a name that has its flags, or none to have -> itself"""
    base, _, args = name.partition("<")
    args = [a.strip() for a in args.rstrip(">").split(",")] if args else []
    last = base.endswith(("_retry", "_listed"))
    if last: base = base[:base.rindex("_")]
    excl = base.endswith("_excl")
    if excl: base = base[:-5]
    if base not in FLAGGED or len(args) == FLAGGED[base][0]: return name
    if base == "k_backward_mfma" and len(args) == 2: args.append("0")          # ABL
    args += (["true" if excl else "false"] if FLAGGED[base][1] else []) + ["true" if last else "false"]
    return base + "<" + ", ".join(args) + ">"


def assemble(tree, out):
    csrc = os.path.join(tree, "trajoptkp_amd", "csrc")
    os.makedirs(out, exist_ok=True)
    todo = []
    for line in subprocess.check_output(["make", "-n", "-B", "-C", csrc, "OBJ=" + out], text=True).splitlines():
        m = re.search(r" -c (.*) -o (\S+)/(\w+)\.o$", line)
        if m and m.group(3) in UNITS and not os.path.exists(os.path.join(out, m.group(3) + ".s")):
            todo.append(line[:m.start()] + " -S --cuda-device-only %s -o %s/%s.s" % m.groups())
    with concurrent.futures.ThreadPoolExecutor(4) as pool:
        for rc in pool.map(lambda cmd: subprocess.call(cmd, shell=True, cwd=csrc, stderr=subprocess.DEVNULL), todo):
            if rc: sys.exit("compilation failed in " + tree)


def kernels(path):
    """{name<args>: normalised text} of the k_backward_* / k_forward_* kernels of one assembly file"""
    text = open(path).read()
    syms = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M)
    names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.splitlines()
    out = {}
    for sym, full in zip(syms, names):
        m = re.search(r"kpilqr::(k_(?:backward|forward)_\w+(?:<[^(]*>)?)\(", full)
        if not m: continue
        body = text[text.index("\n" + sym + ":"):text.index(".end_amdhsa_kernel", text.index(".amdhsa_kernel " + sym + "\n"))]
        lines = (re.sub(r"\.L(BB|func_end|tmp)\d+", r".L\1", l.split(";")[0]).rstrip().replace(sym, "<own symbol>") for l in body.splitlines())
        out[flag_name(m.group(1))] = "\n".join(l for l in lines if l and ".amdhsa_kernarg_size" not in l)
    assert len(out) == sum(1 for f in names if re.search(r"kpilqr::k_(backward|forward)_", f)), "two kernels under one name in " + path
    return out


def main():
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    old_tree, new_tree = sys.argv[1], sys.argv[2]
    tmp = None if keep else tempfile.TemporaryDirectory()
    root = os.path.abspath(keep or tmp.name)
    assemble(old_tree, os.path.join(root, "old"))
    assemble(new_tree, os.path.join(root, "new"))
    bad = 0
    print("%-14s %9s %6s %9s %9s %9s" % ("unit", "compared", "equal", "different", "old only", "new only"))
    for unit in UNITS:
        old = kernels(os.path.join(root, "old", unit + ".s"))
        new = kernels(os.path.join(root, "new", unit + ".s"))
        both = sorted(set(old) & set(new))
        differ = [k for k in both if old[k] != new[k]]
        only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
        print("%-14s %9d %6d %9d %9d %9d" % (unit, len(both), len(both) - len(differ), len(differ), len(only_old), len(only_new)))
        for k in only_old: print("    old only: " + k)
        for k in only_new: print("    new only: " + k)
        for k in differ:
            a, b = old[k].splitlines(), new[k].splitlines()
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("    differs: %s, line %d of %d / %d:\n      old %s\n      new %s" % (k, i, len(a), len(b), a[i:i + 1], b[i:i + 1]))
        bad += len(differ) + len(only_old) + len(only_new)
    print("verdict: " + ("every kernel has its partner and the same text" if not bad else "%d kernels differ or have no partner" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
