"""Timing of on-device key-point placement at the headline shape: Panda, T=3000, B=1024.

  python tools/kp_device_timing.py                      the whole-batch placement, per method
  python tools/kp_device_timing.py partial [--batch B] [--fractions ...] [--samples N] [--whole-only] [--out FILE]
      a scattered fraction of the batch gets new states and new lists (velocity_change(5, 100)), with the key-point ordered payload
      resident.  Two routes bring the context there, on ONE fused context in one process, alternating a b b a ...:
        (a) the whole batch again: kpilqr_upload_states + kpilqr_generate_keypoints + kpilqr_get_keypoints + kpilqr_upload_fd_kp
        (b) kpilqr_upload_states_partial + kpilqr_generate_keypoints_partial + kpilqr_get_keypoints_partial + kpilqr_upload_fd_kp_partial
      Host clock from the first call to the completion of the context's stream; one warm-up round, then --samples (5) timed calls
      each; median and min .. max.  The routes are timed, not iterated on: the pinned slabs hold no finite differences
      (tests/test_gpu_keypoints_partial.py holds the results).  --whole-only times (a) alone: what a library without the new calls
      can run (KPILQR_LIB=<libkpilqr.so of the parent commit>), for the comparison of (a) between the two builds on the same box."""
import argparse
import json
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: trajoptkp_amd._lib)

sys.path.insert(0, ".")
from trajoptkp_amd import Engine  # noqa: E402

T, dof = 3000, 7


def whole_batch(B=1024):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((8, T, 2 * dof)).cumsum(axis=1) * 0.01
    X = np.tile(X, (B // 8, 1, 1))
    with Engine(dof, 7, T, 14, batch=B) as e:
        t0 = time.perf_counter(); e.upload_states(X); e.sync(); up = time.perf_counter() - t0
        for method, thr in (("set_interval", None), ("adaptive_jerk", np.full(dof, 100.0)), ("velocity_change", np.full(dof, 1.0))):
            e.generate_keypoints(method, 5, 100, thr, 0.008); e.sync()
            t0 = time.perf_counter()
            for _ in range(5):
                e.generate_keypoints(method, 5, 100, thr, 0.008)
            e.sync()
            dt = (time.perf_counter() - t0) / 5
            offs, times = e.get_keypoints()
            print(f"{method:16s}: {dt*1e3:7.3f} ms per batch (placement + scan + fill + segmap), {len(times)/(B*dof*T)*100:5.1f} % key-points", flush=True)
        print(f"state upload (pageable, {X.nbytes/1e6:.0f} MB): {up*1e3:.1f} ms")


def stats(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(np.min(ms)), 3), max=round(float(np.max(ms)), 3), n=len(ms))


def partial_leg(args):
    B, N = args.batch, args.samples
    gen = ("velocity_change", 5, 100, np.full(dof, 1.0), 0.008)
    rng = np.random.default_rng(0)
    # two sets of states per trajectory: a listed trajectory toggles between them, so that its lists change length both ways
    Xv = [np.tile(rng.standard_normal((8, T, 2 * dof)).cumsum(axis=1) * 0.01, (B // 8 + 1, 1, 1))[:B] for _ in (0, 1)]
    rows = []
    with Engine(dof, 7, T, 14, batch=B, fused=True) as e:
        stride = (6 * e.n + 2) * 8
        totals = []
        for X in Xv:                                          # the largest payload either set of states asks for
            e.upload_states(X); e.generate_keypoints(*gen)
            totals.append(len(e.get_keypoints()[1]))
        cap = max(totals) + B * dof * 64
        full, part = e.pinned(cap * stride, np.uint8), e.pinned(cap * stride, np.uint8)
        full[:] = 0; part[:] = 0
        # pinned, filled per fraction outside the timed calls: everybody's states with the listed ones toggled | the listed ones, compact
        Xmix, Xsub = [e.pinned(Xv[0].shape) for _ in (0, 1)], [e.pinned(Xv[0].shape) for _ in (0, 1)]
        sel = np.random.default_rng(5)
        for f in args.fractions:
            cnt = max(1, int(round(f * B)))
            traj = np.sort(sel.choice(B, cnt, replace=False)).astype(np.int32)
            listed = np.zeros(B, bool); listed[traj] = True
            for v in (0, 1):
                Xmix[v][...] = Xv[0]; Xmix[v][listed] = Xv[v][listed]
                Xsub[v][:cnt] = Xv[v][listed]
            bytes_up = {}

            def route_a(v):
                e.upload_states(Xmix[v]); e.generate_keypoints(*gen)
                entries = len(e.get_keypoints()[1])
                e.upload_fd_kp(dict(slab=full, entries=entries), eps=1e-6)
                bytes_up["a"] = Xmix[v].nbytes + entries * stride

            def route_b(v):
                e.upload_states_partial(traj, Xsub[v][:cnt]); e.generate_keypoints_partial(traj, *gen)
                entries = len(e.get_keypoints_partial(traj)[1])
                e.upload_fd_kp_partial(traj, dict(slab=part, entries=entries), eps=1e-6)
                bytes_up["b"] = Xsub[v][:cnt].nbytes + entries * stride

            def wall(fn):
                e.sync(); t0 = time.perf_counter(); fn(); e.sync()
                return (time.perf_counter() - t0) * 1e3
            route_a(0); e.sync()
            ms = {"a": [], "b": []}
            v, i = 0, 0
            order = "a" if args.whole_only else "ab"
            while min(len(ms[k]) for k in order) < N + 1:      # a b b a a b b a ...; the first call of each is warm-up
                name = order[((i + 1) // 2) % len(order)]
                v ^= 1
                ms[name].append(wall((lambda: route_a(v)) if name == "a" else (lambda: route_b(v))))
                i += 1
            row = dict(batch=B, T=T, fraction=f, listed=cnt, route_a_ms=stats(ms["a"][1:1 + N]), bytes_a=bytes_up.get("a"))
            if not args.whole_only:
                row.update(route_b_ms=stats(ms["b"][1:1 + N]), bytes_b=bytes_up.get("b"),
                           b_over_a=round(float(np.median(ms["b"][1:1 + N]) / np.median(ms["a"][1:1 + N])), 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
    box = f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}"
    out = [f"box: {box}; Panda reaching, velocity_change(5, 100); B = {B}, T = {T}; (a) whole-batch placement + whole payload | (b) the listed subset; ms, median (min..max) of {N}"]
    for r in rows:
        a = r["route_a_ms"]
        line = f"{r['fraction']:<7.4f} {r['listed']:<6}  (a) {a['median']:8.2f} ({a['min']:.2f}..{a['max']:.2f})  {r['bytes_a'] / 1e6:7.0f} MB"
        if "route_b_ms" in r:
            b = r["route_b_ms"]
            line += f"   (b) {b['median']:8.2f} ({b['min']:.2f}..{b['max']:.2f})  {r['bytes_b'] / 1e6:7.0f} MB   b/a {r['b_over_a']:.3f}"
        out.append(line)
    text = "\n".join(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")
            fh.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", nargs="?", default="whole", choices=["whole", "partial"])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fractions", nargs="*", type=float, default=[1 / 32, 1 / 4, 1 / 2])
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--whole-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    whole_batch(a.batch) if a.leg == "whole" else partial_leg(a)
