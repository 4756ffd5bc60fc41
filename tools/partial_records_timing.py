"""Same-process A/B of the record passes and residual uploads of a partial re-linearisation on the two tiled side workloads of the
bench (bench.py's builders, imported; bench.py untouched):
    pushing    configs[2]  panda_pushing, n = 20, B = 64,  T = 3000, adaptive_jerk lists
    configs4   configs[4]  high_dof_push, n = 62, B = 128, T = 5000, iterative_error lists
python tools/partial_records_timing.py [--workloads pushing configs4] [--fractions ...] [--samples N] [--out FILE]

ONE materialising context per workload with the key-point ordered payload, the residuals and their Jacobians resident.  For a
fraction f of the trajectories (a seeded random subset: the regenerating trajectories of a batch are scattered) three pairs of calls
alternate (whole partial partial whole ...), one warm-up of each, then --samples (5) timed ones, HIP events on the context's stream,
median and min .. max:
    kpilqr_fd_interpolate   | kpilqr_fd_interpolate_partial(subset)
    kpilqr_cost_derivs      | kpilqr_cost_derivs_partial(subset)
    kpilqr_upload_residuals | kpilqr_upload_residuals_partial(subset)       r, r_x, r_u from pinned memory
The list of the partial calls is pinned (no wait inside the call).  Byte model: partial = f x whole.  Condition (a): at f = 1 the
partial median lies inside the whole-batch call's own min .. max of that run.
With a library that lacks the partial calls (KPILQR_LIB naming a build of the parent commit) only the whole-batch columns are timed:
condition (b) compares them between the two builds on one box in one visit, within the parent's min .. max.
Prints one JSON line per (workload, fraction) and a table; --out appends."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from trajoptkp_amd import Engine, _lib, synth  # noqa: E402

WORKLOADS = {"pushing": ("adaptive_jerk", "panda_pushing", 3000, 64, 5), "configs4": ("iterative_error", "high_dof_push", 5000, 128, 3)}


def events(stream, e, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e.sync()
    a.record(stream); fn(); b.record(stream); b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(np.min(ms)), 3), max=round(float(np.max(ms)), 3), n=len(ms))


def alternate(stream, e, whole, part, N):
    """whole part part whole ...: N + 1 of each, the first of each dropped; part None: the whole-batch call alone."""
    ms = {"w": [], "p": []}
    i = 0
    while len(ms["w"]) < N + 1 or (part is not None and len(ms["p"]) < N + 1):
        name = "wp"[((i + 1) // 2) % 2] if part is not None else "w"
        ms[name].append(events(stream, e, whole if name == "w" else part))
        i += 1
    return stats(ms["w"][1:N + 1]), (stats(ms["p"][1:N + 1]) if part is not None else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--fractions", nargs="*", type=float, default=[1 / 16, 1 / 4, 1 / 2, 1.0])
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N = args.samples
    stream = torch.cuda.Stream(); torch.cuda.set_stream(stream)
    L = _lib.load()
    have = hasattr(L, "kpilqr_fd_interpolate_partial")
    rows = []
    for name in args.workloads:
        kind, task, T, B, min_N = WORKLOADS[name]
        p, _, desc = bench.build_problem(kind, B, T, min_N, task, distinct=False)
        n, m, nr = p["n"], p["m"], p["nr"]
        with Engine(p["dof"], m, T, nr, batch=B, stream=stream.cuda_stream) as e:
            synth.upload(e, p, kp_ordered=True)
            pin = {}
            for key in ("r", "r_x", "r_u"):
                pin[key] = e.pinned(p[key].shape); pin[key][...] = p[key]
            ptr = {k: v.ctypes.data for k, v in pin.items()}
            e.upload_residuals(pin["r"], pin["r_x"], pin["r_u"])
            e.fd_interpolate(); e.cost_derivs(); e.sync()
            how = e.last_launch("linearise")
            rng = np.random.default_rng(5)
            tr = e.pinned(B, np.int32)
            for f in args.fractions:
                cnt = max(1, int(round(f * B)))
                tr[:cnt] = np.sort(rng.choice(B, cnt, replace=False))
                tp = tr.ctypes.data
                ck, h = e._ck, e._h
                pairs = {
                    "fd_interpolate": (lambda: ck(L.kpilqr_fd_interpolate(h)), lambda: ck(L.kpilqr_fd_interpolate_partial(h, cnt, tp))),
                    "cost_derivs": (lambda: ck(L.kpilqr_cost_derivs(h)), lambda: ck(L.kpilqr_cost_derivs_partial(h, cnt, tp))),
                    "upload_residuals": (lambda: ck(L.kpilqr_upload_residuals(h, ptr["r"], ptr["r_x"], ptr["r_u"], None, None)),
                                         lambda: ck(L.kpilqr_upload_residuals_partial(h, cnt, tp, ptr["r"], ptr["r_x"], ptr["r_u"]))),
                }
                row = dict(workload=name, desc=desc, batch=B, T=T, n=n, fraction=f, listed=cnt, linearise=how, partial_calls=have,
                           residual_bytes_whole=int(sum(v.nbytes for v in pin.values())),
                           residual_bytes_partial=int(sum(v.nbytes for v in pin.values()) // B * cnt))
                for key, (whole, part) in pairs.items():
                    w, q = alternate(stream, e, whole, part if have else None, N)
                    row[key + "_whole_ms"] = w
                    if q is not None:
                        row[key + "_partial_ms"] = q
                        row[key + "_ratio"] = round(q["median"] / w["median"], 4)
                        if f == 1.0:
                            row[key + "_condition_a"] = bool(w["min"] <= q["median"] <= w["max"])
                rows.append(row)
                print(json.dumps(row), flush=True)
                if not have:
                    break                  # (the whole-batch calls do not depend on the fraction)
    box = f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}, {os.path.basename(_lib.LIB_PATH)} with{'' if have else 'OUT'} the partial calls"
    out = [f"box: {box}; ms, median (min..max) of {N}; whole | partial, partial / whole",
           "workload  f       listed  fd_interpolate                                        cost_derivs                                           upload_residuals (r, r_x, r_u)"]
    for r in rows:
        cells = []
        for key in ("fd_interpolate", "cost_derivs", "upload_residuals"):
            w, q = r[key + "_whole_ms"], r.get(key + "_partial_ms")
            cell = f"{w['median']:8.3f} ({w['min']:.3f}..{w['max']:.3f})"
            if q:
                cell += f" | {q['median']:8.3f} ({q['min']:.3f}..{q['max']:.3f}) {r[key + '_ratio']:.3f}"
                if key + "_condition_a" in r:
                    cell += " (a) " + ("ok" if r[key + "_condition_a"] else "OUTSIDE")
            cells.append(cell)
        out.append(f"{r['workload']:<9} {r['fraction']:<7.4f} {r['listed']:<6}  " + "   ".join(cells))
    text = "\n".join(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
