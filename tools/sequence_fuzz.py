"""Randomised sequence sweep on the GPU box: python tools/sequence_fuzz.py [--seed S] [--count N] [--kind K] [--ops M].
The command-line twin of tools/fuzz_parity.py for tests/_sequences.py: N random sequences of M ops on one long-lived context each
(the kinds in turn, or --kind alone), every observation compared with the CPU oracle (1e-9) and with a fresh context (bit for bit
where both ran the same forms, 1e-12 otherwise).  The committed seeds run in the -m gpu suite (tests/test_gpu_sequences.py); this
is for seeds outside that list.  A failing sequence is printed as its op list, ready to be cut by hand and kept as a reduced case."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import _sequences as Q

ap = argparse.ArgumentParser()
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--count", type=int, default=20)
ap.add_argument("--kind", choices=list(Q.KINDS))
ap.add_argument("--ops", type=int, default=Q.N_OPS)
args = ap.parse_args()

kinds = [args.kind] if args.kind else list(Q.KINDS)
per_launch, total = {}, dict(observations=0, bit_equal=0, form_compared=0, worst_forms=0.0)
t0 = time.time()
for i in range(args.count):
    kind = kinds[i % len(kinds)]
    ops = Q.draw_sequence(np.random.default_rng([args.seed, i]), kind, args.ops, min_obs=max(1, args.ops // 4))
    st = Q.run_sequence(kind, ops, tag=f"sequence {i} ({kind}, --seed {args.seed})")
    for launch, errs in st["per_launch"].items():
        w = per_launch.setdefault(launch, {})
        for k, v in errs.items():
            w[k] = max(w.get(k, 0.0), v)
    for k in ("observations", "bit_equal", "form_compared"):
        total[k] += st[k]
    total["worst_forms"] = max(total["worst_forms"], st["worst_forms"])
    print(f"sequence {i:3d} {kind:14s} {st['observations']:2d} observations, {len(st['launches'])} launch strings  ok", flush=True)
print(f"{args.count} sequences of {args.ops} ops (seed {args.seed}) in {time.time() - t0:.1f} s: {total['observations']} observations, none skipped")
print(f"against a fresh context: {total['bit_equal']} observations bit-equal, {total['form_compared']} compared at {Q.RTOL_FORMS:g} "
      f"(other launch strings; worst {total['worst_forms']:.1e})")
print(f"worst relative errors against the oracle per backward launch string (bar {Q.RTOL:g}):")
for launch, w in sorted(per_launch.items()):
    print(f"  {launch:55s} " + " ".join(f"{k}={v:.1e}" for k, v in sorted(w.items())))
