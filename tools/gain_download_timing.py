"""Timing of the gain download into pinned memory, FP64 (kpilqr_download_gains / _partial) against FP32
(kpilqr_download_gains_f32 / _partial), with events on the context's stream: the whole batch and a scattered half (every other
trajectory: no two adjacent, so the FP64 route makes one copy per trajectory and array).

    python tools/gain_download_timing.py [--reps N] [--out FILE] [--kernel-trace DIR]

The FP64 calls are the baseline: the same code as before the FP32 calls existed, in the same process on the same box.  Both routes
are timed alternately.  K alone is timed as well as K with k, which is the same FP64 copy on both routes.

The conversion kernel's own time does not come from the events (a call is kernel + copy): run the tool once under
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gain_download_timing.py --reps 3 --f32-only
and give the directory to a second, unprofiled run with --kernel-trace DIR; the dispatches of k_gains_f32 are matched to the cases
by their grid.

Gains are random (16 distinct trajectories tiled over the batch) and injected into KPILQR_BUF_K; every FP32 result is checked
against the cast of the FP64 download."""
import argparse
import csv
import ctypes as C
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajoptkp_amd import Engine  # noqa: E402

# name, dof, m, batch, T, fused (a fused context holds no step records: 14 GB less at the Panda shape)
CASES = [("panda", 7, 7, 1024, 3000, True), ("n=20 tiled", 10, 7, 64, 3000, False)]
THREADS, ITERS = 256, 8           # KPG_THREADS, KPG_ITERS of csrc/gains.hip: the grid of a launch follows from them


def event_ms(stream, fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(); b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def kernel_times(trace_dir):
    """{(grid threads x, grid threads y): [ms, ...]} of every k_gains_f32 dispatch in a rocprofv3 kernel-trace directory"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "k_gains_f32" not in row.get("Kernel_Name", ""):
                continue
            key = (int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]))
            out.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    return out


def run(name, dof, m, B, T, fused, reps, f32_only, ktimes, lines):
    rng = np.random.default_rng(dof * 1000 + B)
    n = 2 * dof
    K16 = rng.standard_normal((16, T, n, m)) * np.exp(rng.uniform(-3, 2, (16, 1, n, 1)))
    stream = torch.cuda.Stream()
    with Engine(dof, m, T, 2, batch=B, stream=stream.cuda_stream, fused=fused) as e:
        dev = torch.as_tensor(e.device_array(1, (B, T, n, m)), device="cuda")
        with torch.cuda.stream(stream):
            for i in range(0, B, 16):
                dev[i:i + 16].copy_(torch.from_numpy(K16))
        stream.synchronize()
        L, h = e._L, e._h
        K64 = e.pinned((B, T, n, m)); K32 = e.pinned((B, T, n, m), np.float32); k = e.pinned((B, T, m))
        half = e.pinned(B // 2, np.int32); half[:] = np.arange(0, B, 2)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        calls = {
            ("whole", "K"): (lambda: e._ck(L.kpilqr_download_gains(h, p(K64), None)), lambda: e._ck(L.kpilqr_download_gains_f32(h, p(K32), None))),
            ("whole", "K+k"): (lambda: e._ck(L.kpilqr_download_gains(h, p(K64), p(k))), lambda: e._ck(L.kpilqr_download_gains_f32(h, p(K32), p(k)))),
            ("half", "K"): (lambda: e._ck(L.kpilqr_download_gains_partial(h, B // 2, p(half), p(K64), None)),
                            lambda: e._ck(L.kpilqr_download_gains_f32_partial(h, B // 2, p(half), p(K32), None))),
            ("half", "K+k"): (lambda: e._ck(L.kpilqr_download_gains_partial(h, B // 2, p(half), p(K64), p(k))),
                              lambda: e._ck(L.kpilqr_download_gains_f32_partial(h, B // 2, p(half), p(K32), p(k)))),
        }
        per = T * n * m
        ref16 = K16.astype(np.float32)
        for (which, what), (f64, f32) in calls.items():
            rows = B if which == "whole" else B // 2
            K32.fill(0)
            f32(); e.sync()                                        # the float buffer is reserved, code objects are loaded
            step = 1 if which == "whole" else 2                    # (16 distinct trajectories tiled over the batch)
            assert np.array_equal(K32[:rows].reshape(-1, 16 // step, T, n, m).view(np.uint32), np.broadcast_to(ref16[::step].view(np.uint32), (rows * step // 16, 16 // step, T, n, m))), (name, which)
            if f32_only:
                for _ in range(reps):
                    f32()
                e.sync()
                continue
            f64(); e.sync()
            t64, t32 = [], []
            for _ in range(reps):                                  # alternating: both routes see the same box
                t64.append(event_ms(stream, f64, 1)[0]); t32.append(event_ms(stream, f32, 1)[0])
            m64, m32 = float(np.median(t64)), float(np.median(t32))
            b64 = rows * (per * 8 + (T * m * 8 if what == "K+k" else 0)); b32 = rows * (per * 4 + (T * m * 8 if what == "K+k" else 0))
            grid = (min(4096, -(-(per // 2) // (THREADS * ITERS))) * THREADS, min(rows, 65535))
            kt = ktimes.get(grid)
            kern = f"kernel {np.median(kt):6.3f} ms ({rows * per * 12 / np.median(kt) / 1e9:5.2f} TB/s over 12 B per element, {len(kt)} dispatches)" if kt else "kernel not traced"
            line = (f"{name:10s} n={n:2d} m={m} B={B:4d} T={T} {which:5s} {what:3s}: FP64 {b64 / 1e9:6.3f} GB {m64:8.3f} ms (min {min(t64):8.3f}, "
                    f"{b64 / m64 / 1e6:5.1f} GB/s) | FP32 {b32 / 1e9:6.3f} GB {m32:8.3f} ms (min {min(t32):8.3f}, {b32 / m32 / 1e6:5.1f} GB/s) | "
                    f"FP32 / FP64 {m32 / m64:.3f} | {kern}")
            print(line, flush=True)
            lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--f32-only", action="store_true", help="only the FP32 calls, untimed: the run to put under rocprofv3 --kernel-trace")
    ap.add_argument("--kernel-trace", default=None, help="directory of that profiled run: adds k_gains_f32's own time to every line")
    a = ap.parse_args()
    ktimes = kernel_times(a.kernel_trace) if a.kernel_trace else {}
    lines = [f"# {torch.cuda.get_device_name(0)}; pinned destinations; median of {a.reps} event-timed calls per route, the two routes alternating"]
    for c in CASES:
        run(*c, a.reps, a.f32_only, ktimes, lines)
    if a.out and not a.f32_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
