"""Which compiled sweep kernels a test run dispatched: python tools/shape_coverage.py STATS.csv [--before STATS0.csv] > out.txt

Lists the kernel symbols of the sweep translation units (hipcc --cuda-device-only -S with the Makefile's flags, as
tools/isa_lint.py does; fused_mfma.hip once per KP_FUSED_PART), reads the kernel names of a `rocprofv3 --kernel-trace --stats
--output-format csv` run (its *_kernel_stats.csv), and prints every symbol as dispatched (with its count) or not, with the reason
for each one not dispatched (REASONS below; a symbol with no reason is marked UNEXPLAINED and the exit status is 1).  --before:
the stats of a run of the suite without tests/test_gpu_shapes.py; symbols it did not dispatch are marked NEW."""
import csv, glob, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trajoptkp_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function"]
MFMAF = ["-mllvm", "-amdgpu-mfma-vgpr-form"]
UNITS = [("riccati_mfma.hip", MFMAF), ("forward_mfma.hip", MFMAF), ("tiled_mfma.hip", MFMAF), ("tiled_wide.hip", MFMAF),
         ("generic.hip", ["-ffp-contract=off"])] + [("fused_mfma.hip", MFMAF + [f"-DKP_FUSED_PART={i}"]) for i in (1, 2, 3)]

# (pattern on the demangled name, reason it is not dispatched by tests/test_gpu_shapes.py)
# The trailing template flags of the sweep kernels are ..., EXCL, GATED backward and ..., EXCL, LISTED forward (the
# pair, triple and tiled kernels have no EXCL; generic.hip keeps the name suffixes _retry / _listed).  First match wins.
REASONS = [
    (r"k_backward_\w+<.*, true>$|k_backward_generic_retry\b", "GATED instantiation, the lambda retry twin (kpilqr_set_lambda_retry): runs the attempts behind the "
                                                             "first of a backward pass under a schedule; tests/test_gpu_lambda_retry.py dispatches one per family"),
    (r"k_forward_\w+<.*, true>$|k_forward_generic_listed\b", "LISTED instantiation (kpilqr_forward_linear_partial): sweeps a listed subset of the batch; "
                                                            "tests/test_gpu_partial_sweeps.py dispatches one per family"),
    (r"k_backward_fused_stats<", "diagnostic entry point only (kpilqr_backward_stats, the refresh histogram)"),
    (r"k_(backward|forward)_fused<.*, false, false>$", "plain form (EXCL = false: batch > n_simd) in a residual / payload mode other than the headline's (constant r_x, "
                                                       "key-point ordered payload): test_batch_boundaries runs the plain form in that mode only"),
    (r"k_(backward_fused|backward_fusedph|forward_fused|forward_fused_sc3|forward_fused_scu)<",
     "a residual / payload mode of the fused sweeps (template flags RU / RW / UN / RX / SL), not a shape: the shape cases run "
     "dense r_u or a constant r_x, never r_u = 0 with per-step r_x"),
]


def symbols():
    out = {}
    for src, extra in UNITS:
        with tempfile.TemporaryDirectory() as td:
            s = os.path.join(td, "k.s")
            subprocess.check_call(["hipcc"] + FLAGS + extra + ["-S", "--cuda-device-only", "-o", s, os.path.join(CSRC, src)],
                                  stderr=subprocess.DEVNULL)
            for line in open(s):
                m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
                if m:
                    out[m.group(1)] = src
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return [(sym, dem, out[sym]) for sym, dem in zip(out, names)]


def _key(name):
    """A demangled kernel name without its return type and parameter list (rocprofv3 and c++filt agree on the rest)."""
    name = name.strip()
    if name.startswith("void "):
        name = name[5:]
    depth = 0
    for i, ch in enumerate(name):
        if ch == "<": depth += 1
        elif ch == ">": depth -= 1
        elif ch == "(" and depth == 0: return re.sub(r"\s+", " ", name[:i])
    return re.sub(r"\s+", " ", name)


def dispatched(path):
    counts = {}
    files = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True) if os.path.isdir(path) else [path]
    for f in files:
        for row in csv.DictReader(open(f)):
            counts[_key(row["Name"])] = counts.get(_key(row["Name"]), 0) + int(row.get("Calls", 1))
    return counts


def horizon_residues(n_simd=1024):
    """Per time loop of tests/_horizons.py: its step group and the residues T mod group, and the horizons below one group, that the
    cases of tests/_shapes.py and of tests/_horizons.py run it at."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _horizons as HZ, _shapes as S
    lines = []
    for loop, g in sorted(HZ.GROUPS.items()):
        for name, cs in (("_shapes", [c for c in S.cases(n_simd) if c["why"] != "refused"]), ("_horizons", HZ.cases())):
            Ts = sorted({c["T"] for c in cs if loop in HZ.loops_of(c, n_simd)})
            lines.append(f"# loop {loop} (group {g}) {name}: residues {sorted({T % g for T in Ts if T >= g})}, below a group {[T for T in Ts if T < g]}")
    return lines


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    before = dispatched(sys.argv[sys.argv.index("--before") + 1]) if "--before" in sys.argv else None
    if before is not None:
        args.remove(sys.argv[sys.argv.index("--before") + 1])
    now = dispatched(args[0])
    syms = symbols()
    bad = 0
    n_new = n_hit = 0
    lines = []
    for sym, dem, src in sorted(syms, key=lambda x: (x[2], _key(x[1]))):
        k = _key(dem)
        if now.get(k):
            n_hit += 1
            new = before is not None and not before.get(k)
            n_new += new
            lines.append(f"{'NEW ' if new else ''}dispatched {now[k]:6d}  {k}  [{src}]")
        else:
            why = next((r for p, r in REASONS if re.search(p, k)), None)
            bad += why is None
            also = " (the rest of the GPU suite dispatches it)" if before is not None and before.get(k) else ""
            lines.append(f"not dispatched  {k}  [{src}]: {why or 'UNEXPLAINED'}{also}")
    print(f"# {len(syms)} sweep kernels compiled, {n_hit} dispatched by tests/test_gpu_shapes.py"
          + (f", {n_new} of them (NEW) by no other test of the GPU suite" if before is not None else "") + f"; {bad} unexplained")
    print("\n".join(lines))
    print("\n".join(horizon_residues()))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
