"""Timing of the two ways the per-step residual Jacobians of a linearisation reach the device, in one process, alternating: as FP64
(kpilqr_upload_residuals(NULL, r_x, r_u, ...), or kpilqr_upload_residuals_partial for a subset) and as FP32
(kpilqr_upload_residual_jacobians_f32[_partial]: one copy per array into the staging buffer + the widening launches), from pinned
memory, with events on the context's stream, on the headline shape: Panda reaching, T = 3000, nr = 14, dense_residuals="smooth"
(4.71 MB of r_x and 2.35 MB of r_u per trajectory as FP64).  Whole batch, and a scattered quarter of it (every fourth trajectory).

    python tools/residual_jacobians_f32_timing.py [--batch B] [--reps N] [--warmup W] [--out FILE]

The Jacobians are one trajectory's (synth.make_problem) tiled over the batch: a transfer does not care.  What an event pair brackets
is the upload call alone; after either route the r_x / r_u buffers hold what the sweeps read.  Before anything is timed the FP32 route
is checked against the FP64 route on the widened doubles on a small batch (K and k behind kpilqr_iterate, bit for bit).  A run needs
a GPU; without one the tool fails.  The table of profiles/residual_jacobians_f32.txt (section 3) is this tool's output."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajoptkp_amd import Engine, synth  # noqa: E402

TASK, T, MIN_N = "panda_reaching", 3000, 5


def event_ms(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream); fn(); b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def check_small():
    """The FP32 route against the FP64 route on the widened doubles: K and k of one iteration, three trajectories at T = 300, a whole
    upload followed by rows of trajectories 0 and 2"""
    p = synth.make_problem(task=TASK, T=300, batch=3, min_N=MIN_N, dense_residuals=True)
    x32, u32 = synth.residual_jacobians_f32(p)
    dx, du = x32.astype(np.float64), u32.astype(np.float64)
    tr = [0, 2]
    out = []
    for f32 in (False, True):
        with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=3, fused=True) as e:
            synth.upload(e, p)
            if f32:
                e.upload_residual_jacobians_f32(x32, u32)
                e.upload_residual_jacobians_f32(x32[[1, 0]], u32[[1, 0]], traj=tr)
            else:
                e.upload_residuals(None, dx, du)
                e.upload_residuals_partial(tr, None, dx[[1, 0]], du[[1, 0]])
            e.iterate(p["lam"], 100, (np.arange(1, 7) / 6.0) ** 2)
            out.append(e.gains())
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("residual_jacobians_f32_timing: no GPU (nothing is timed on a CPU)")
    if a.reps < 10:
        sys.exit("residual_jacobians_f32_timing: at least 10 runs per route")
    check_small()
    B = a.batch
    p = synth.make_problem(task=TASK, T=T, batch=1, min_N=MIN_N, dense_residuals="smooth")
    dof, n, m, nr = p["dof"], p["n"], p["m"], p["nr"]
    x32_1, u32_1 = synth.residual_jacobians_f32(p)
    traj = np.arange(1, B, 4, dtype=np.int32)                      # a scattered quarter: no two listed trajectories are adjacent
    C = len(traj)
    stream = torch.cuda.Stream()
    with Engine(dof, m, T, nr, batch=B, stream=stream.cuda_stream, fused=True) as e:
        rx = e.pinned((B, T + 1, nr, n)); rx[:] = p["r_x"][0]
        ru = e.pinned((B, T + 1, nr, m)); ru[:] = p["r_u"][0]
        x32 = e.pinned((B, T + 1, nr, n), np.float32); x32[:] = x32_1[0]
        u32 = e.pinned((B, T + 1, nr, m), np.float32); u32[:] = u32_1[0]
        per = (T + 1) * nr * (n + m)
        routes = {
            "whole batch": {
                "FP64 (kpilqr_upload_residuals)": (lambda: e.upload_residuals(None, rx, ru), B * per * 8),
                "FP32 (kpilqr_upload_residual_jacobians_f32)": (lambda: e.upload_residual_jacobians_f32(x32, u32), B * per * 4),
            },
            f"a scattered quarter ({C} of {B} trajectories, every fourth)": {
                "FP64 (kpilqr_upload_residuals_partial)": (lambda: e.upload_residuals_partial(traj, None, rx[:C], ru[:C]), C * per * 8),
                "FP32 (kpilqr_upload_residual_jacobians_f32_partial)": (lambda: e.upload_residual_jacobians_f32(x32[:C], u32[:C], traj=traj), C * per * 4),
            },
        }
        lines = [f"# {torch.cuda.get_device_name(0)}; Panda reaching T={T}, nr={nr}, n={n}, m={m}, dense_residuals=\"smooth\", batch {B}; r_x and r_u together, "
                 f"pinned sources; median of {a.reps} event-timed calls per route after {a.warmup} warm-up rounds, the two routes alternating"]
        for title, pair in routes.items():
            for _ in range(a.warmup):                              # code objects loaded, the staging buffer reserved
                for fn, _b in pair.values():
                    fn()
            e.sync()
            times = {k: [] for k in pair}
            for _ in range(a.reps):                                # alternating: both routes see the same machine
                for k, (fn, _b) in pair.items():
                    times[k].append(event_ms(stream, fn))
            e.sync()
            base = float(np.median(next(iter(times.values()))))
            lines.append(f"{title}")
            for k, (_fn, nbytes) in pair.items():
                t = np.asarray(times[k]); med = float(np.median(t))
                lines.append(f"  {k:52s} {nbytes / 1e9:6.3f} GB: median {med:8.3f} ms (min {t.min():8.3f}, max {t.max():8.3f}), "
                             f"{nbytes / med / 1e6:5.1f} GB/s of payload, {med / base:.3f} of the FP64 route's time")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
