"""Timing of the three ways the dynamics of a linearisation reach the device, in one process, alternating: the x+ / x- payload
(kpilqr_upload_fd_kp), the FP64 key-point columns (kpilqr_upload_kp_columns) and the FP32 key-point columns
(kpilqr_upload_kp_columns_f32: copy into the staging buffer + the widening launch), from pinned memory, with events on the context's
stream, on the headline shape: Panda reaching, T = 3000, key-points every 5 steps (4 207 entries per trajectory).

    python tools/columns_upload_timing.py [--batch B] [--reps N] [--warmup W] [--out FILE]

The payload is one trajectory's (synth.make_problem) tiled over the batch: a transfer does not care.  What an event pair brackets is
the upload call alone -- for the two column routes everything the sweeps need is then in the column store; the x+ / x- payload is
differenced later (by the raw backward sweep or k_fd_kp_difference), which is NOT in its number.  Before anything is timed the FP32
upload is checked against the FP64 upload of the decoded doubles on a small batch (kpilqr_get_AB behind kpilqr_fd_interpolate,
bit for bit).  A run needs a GPU; without one the tool fails."""
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
    """The FP32 route against the FP64 route on the decoded doubles, A and B of every step, two trajectories at T = 300"""
    p = synth.make_problem(task=TASK, T=300, batch=2, min_N=MIN_N)
    dofs = synth.kp_entry_dofs(p)
    c32 = synth.kp_columns_f32(p)
    dec = synth.decode_kp_columns_f32(c32, dofs, p["dof"])
    out = []
    for up in (lambda e: e.upload_kp_columns(dict(cols=dec, entries=len(dec))), lambda e: e.upload_kp_columns_f32(c32)):
        with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=2) as e:
            e.set_keypoints_rows(p["kp_rows"])
            up(e)
            e.fd_interpolate()
            out.append(e.get_AB())
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("columns_upload_timing: no GPU (nothing is timed on a CPU)")
    check_small()
    B = a.batch
    p = synth.make_problem(task=TASK, T=T, batch=1, min_N=MIN_N)
    dof, n = p["dof"], p["n"]
    xp, xm, mode = synth.kp_ordered_payload(p)
    E1 = len(mode); E = E1 * B
    c32_1 = synth.kp_columns_f32(p); cols_1 = synth.kp_columns(p)
    stream = torch.cuda.Stream()
    with Engine(dof, p["m"], T, p["nr"], batch=B, stream=stream.cuda_stream, fused=True) as e:
        e.set_keypoints_rows(p["kp_rows"] * B)
        slab = e.fd_kp_slab(np.tile(xp, (B, 1, 1)), np.tile(xm, (B, 1, 1)), np.tile(mode, B))            # pinned
        cols = e.pinned((E, 3, n)); cols[:] = np.tile(cols_1, (B, 1, 1))
        c32 = e.pinned((E, 3, n), np.float32); c32[:] = np.tile(c32_1, (B, 1, 1))
        routes = {
            "x+ / x- payload (kpilqr_upload_fd_kp)": (lambda: e.upload_fd_kp(slab, eps=p["eps"]), slab["layout"].bytes),
            "FP64 columns (kpilqr_upload_kp_columns)": (lambda: e.upload_kp_columns(dict(cols=cols, entries=E)), E * 3 * n * 8),
            "FP32 columns (kpilqr_upload_kp_columns_f32)": (lambda: e.upload_kp_columns_f32(c32), E * 3 * n * 4),
        }
        for _ in range(a.warmup):                                  # code objects loaded, staging buffer and column store reserved
            for fn, _b in routes.values():
                fn()
        e.sync()
        times = {k: [] for k in routes}
        for _ in range(a.reps):                                    # alternating: every route sees the same machine
            for k, (fn, _b) in routes.items():
                times[k].append(event_ms(stream, fn))
        e.sync()
    lines = [f"# {torch.cuda.get_device_name(0)}; Panda reaching T={T}, key-points every {MIN_N} steps, {E1} entries per trajectory, batch {B}; "
             f"pinned sources; median of {a.reps} event-timed calls per route after {a.warmup} warm-up rounds, the routes alternating"]
    base = float(np.median(times["FP64 columns (kpilqr_upload_kp_columns)"]))
    for k, (_fn, nbytes) in routes.items():
        t = np.asarray(times[k]); med = float(np.median(t))
        lines.append(f"{k:46s} {nbytes / B / 1e6:5.2f} MB per trajectory, {nbytes / 1e9:6.3f} GB: median {med:8.3f} ms (min {t.min():8.3f}, max {t.max():8.3f}), "
                     f"{nbytes / med / 1e6:5.1f} GB/s of payload, {med / base:.3f} of the FP64 columns' time")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
