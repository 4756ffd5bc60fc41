#!/usr/bin/env python3
"""lib_bit_identity.py LIB_A LIB_B [--batch 1024] [--T 3000] [--max-rel]: do two builds of libkpilqr.so compute the same BITS?  (GPU box)

For a change that is meant to move no arithmetic (register and control-flow work in a sweep).  Each library runs in a process of its
own (KPILQR_LIB is read when the package is imported) on the same workload -- bench.py's distinct seeds, Panda reaching, key-points
every 5 steps, from KPILQR_WORKLOAD_CACHE if set -- one backward sweep at the bench's pd_stride and one forward sweep per leg:

    rxc        constant residual Jacobian (the headline)        per_step   residual Jacobians given per step

and leaves SHA-256 digests of the bytes of K, k, delta_J, status and cost_pred of the WHOLE batch (K alone is 2.4 GB at the headline:
only digests leave the process) together with the form the library launched.  Equal digests are equal arrays, bit for bit -- the
comparison is stricter than np.array_equal only in that it tells -0.0 from 0.0 and one NaN payload from another.
Exit status 1 if any digest differs.

--max-rel (for a change that re-orders a sum; use a batch whose arrays fit beside each other, e.g. --batch 64): the arrays are KEPT
(.npy in a temporary directory) and the worst relative difference of every array, max |A - B| / max |A|, is printed beside the digests;
status must still be equal.  Exit status 1 if a status differs or a figure is not finite."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("K", "k", "delta_J", "status", "cost_pred")


def child(batch, T, keep=None):
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    p = bench.distinct_problem("panda_reaching", T, batch, 5, cache=os.environ.get("KPILQR_WORKLOAD_CACHE"))
    from trajoptkp_amd import Engine, synth
    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = {}
    for leg, rxc in (("rxc", True), ("per_step", False)):
        with Engine(p["dof"], p["m"], T, p["nr"], batch=batch, device=0, fused=True) as eng:
            synth.upload(eng, p, kp_ordered=True, rx_const=rxc)
            st, dJ = eng.backward(np.full(batch, p["lam"]), 100)
            launched = eng.last_launch("backward")
            K, k = eng.gains()
            cost = eng.forward_linear(np.array([(i / 6.0) ** 2 for i in range(1, 7)]))
        arrays = dict(zip(NAMES, (K, k, np.asarray(dJ, np.float64), np.asarray(st, np.int32), np.asarray(cost, np.float64))))
        out[leg] = {"backward": launched, "valid": int((np.asarray(st) == 0).sum()), **{n: digest(a) for n, a in arrays.items()}}
        if keep:
            for n, a in arrays.items(): np.save(os.path.join(keep, "%s_%s.npy" % (leg, n)), a)
        del K, k
    print("DIGESTS " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--T", type=int, default=3000)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--max-rel", action="store_true")
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    if args.child: return child(args.batch, args.T, args.keep)
    if len(args.libs) != 2: sys.exit(__doc__)
    got = []
    tmp = tempfile.TemporaryDirectory() if args.max_rel else None
    for i, lib in enumerate(args.libs):
        keep = []
        if tmp:
            os.mkdir(os.path.join(tmp.name, "AB"[i]))
            keep = ["--keep", os.path.join(tmp.name, "AB"[i])]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--batch", str(args.batch), "--T", str(args.T)] + keep,
                           env=dict(os.environ, KPILQR_LIB=os.path.abspath(lib)), capture_output=True, text=True)
        line = next((l for l in r.stdout.splitlines() if l.startswith("DIGESTS ")), None)
        if r.returncode or line is None:
            sys.exit("%s: the run failed (exit status %d)\n%s" % (lib, r.returncode, r.stderr[-2000:]))
        got.append(json.loads(line[8:]))
    bad = 0
    print("batch %d, T %d, Panda reaching, key-points every 5 steps, pd_stride 100; A = %s, B = %s" % (args.batch, args.T, *args.libs))
    for leg in got[0]:
        a, b = got[0][leg], got[1][leg]
        same = [n for n in NAMES if a[n] == b[n]]
        bad += len(NAMES) - len(same) + (a["backward"] != b["backward"])
        print("  %-8s A %s | B %s; valid backward passes %d | %d" % (leg, a["backward"], b["backward"], a["valid"], b["valid"]))
        for n in NAMES: print("    %-9s %s  %s" % (n, a[n][:16], "identical" if a[n] == b[n] else "DIFFERS (B: %s)" % b[n][:16]))
    print("verdict: " + ("every array of every leg is bit-identical" if not bad else "%d arrays or forms differ" % bad))
    if tmp:
        import numpy as np
        worst, ok = 0.0, True
        for leg in got[0]:
            for n in NAMES:
                a, b = (np.load(os.path.join(tmp.name, d, "%s_%s.npy" % (leg, n))) for d in "AB")
                if n == "status":
                    ok = ok and bool(np.array_equal(a, b))
                    print("  %-8s %-9s %s" % (leg, n, "equal" if np.array_equal(a, b) else "DIFFERS"))
                    continue
                rel = float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(a))), 1e-300))
                worst, ok = max(worst, rel), ok and bool(np.isfinite(rel))
                print("  %-8s %-9s max |A - B| / max |A| = %.3e" % (leg, n, rel))
        print("worst relative difference %.3e" % worst)
        return 0 if ok else 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
