#!/usr/bin/env python3
"""lib_bit_identity.py LIB_A LIB_B [--batch 1024] [--T 3000]: do two builds of libkpilqr.so compute the same BITS?  (GPU box)

For a change that is meant to move no arithmetic (register and control-flow work in a sweep).  Each library runs in a process of its
own (KPILQR_LIB is read when the package is imported) on the same workload -- bench.py's distinct seeds, Panda reaching, key-points
every 5 steps, from KPILQR_WORKLOAD_CACHE if set -- one backward sweep at the bench's pd_stride and one forward sweep per leg:

    rxc        constant residual Jacobian (the headline)        per_step   residual Jacobians given per step

and leaves SHA-256 digests of the bytes of K, k, delta_J, status and cost_pred of the WHOLE batch (K alone is 2.4 GB at the headline:
only digests leave the process) together with the form the library launched.  Equal digests are equal arrays, bit for bit -- the
comparison is stricter than np.array_equal only in that it tells -0.0 from 0.0 and one NaN payload from another.
Exit status 1 if any digest differs."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("K", "k", "delta_J", "status", "cost_pred")


def child(batch, T):
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
        del K, k
    print("DIGESTS " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--T", type=int, default=3000)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child: return child(args.batch, args.T)
    if len(args.libs) != 2: sys.exit(__doc__)
    got = []
    for lib in args.libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--batch", str(args.batch), "--T", str(args.T)],
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
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
