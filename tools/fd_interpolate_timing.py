"""Times the linearisation stage (a2 + a4: key-point ordered FD payload -> A, B of every step record) ALONE, with HIP events on the
context's stream: python tools/fd_interpolate_timing.py [cfg2] [cfg4] [panda] [--reps N] [--out FILE]

  cfg2   BASELINE configs[2]: panda_pushing n=20, B=64, T=3000, adaptive-jerk lists
  cfg4   BASELINE configs[4]: high_dof_push n=62, B=128, T=5000, iterative-error lists
  panda  panda_reaching n=14 WITHOUT KPILQR_FLAG_FUSED (bench.py --unfused), B=1024, T=3000, set_interval(5)

The stage is what the library under KPILQR_LIB has: kpilqr_fd_interpolate where the symbol exists (and, beside it, the same
library's separate passes under KPILQR_FD_INTERP=0), else kpilqr_fd_difference + kpilqr_interpolate.  A library built from the
parent commit (tools/build_variant.sh in a checkout of it) is the A/B baseline: run this tool once per library, same box, same
visit (tools/ab_bench.sh's procedure).

Every repetition starts from a payload that has just been uploaded (kpilqr_upload_fd_kp outside the timed region): that is the
state of a real iteration, and it is the only state in which the separate passes difference at all -- a second
kpilqr_fd_difference on an unchanged payload finds the column store valid and only scatters it.  One warm-up repetition, then
the median of --reps.  The one-pass form is also timed launched back to back on the resident payload (no upload in between).

Bytes by the model of DESIGN.md section 9 (E key-point entries, S steps, n, m, c = columns per DoF present in B):
  separate passes  payload E (6n+2) 8 read + kpc E 3n 8 written, read, + key-point columns written, + per 16-step tile and
                   column the two endpoints read from the records, + every in-between element written
  one pass         payload read (once per tile that touches the entry) + every element of a covered step written
Prints one JSON line per workload."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from trajoptkp_amd import Engine, synth  # noqa: E402
from trajoptkp_amd.engine import rows_to_dof_csr  # noqa: E402

WORKLOADS = {
    "cfg2": dict(kind="adaptive_jerk", task="panda_pushing", T=3000, B=64, min_N=5),
    "cfg4": dict(kind="iterative_error", task="high_dof_push", T=5000, B=128, min_N=3),
    "panda": dict(kind="set_interval", task="panda_reaching", T=3000, B=1024, min_N=5),
}
TILE = 16


def build(w):
    """The workload's few distinct trajectories (bench.build_problem's) and, tiled over the batch, its key-point CSR and one
    pageable slab of the key-point ordered payload -- tiled as BYTES: the job lists of the full batch are never formed."""
    uniq = 8 if w["kind"] != "iterative_error" else 2
    _, p0, desc = bench.build_problem(w["kind"], uniq, w["T"], w["min_N"], w["task"], distinct=False)
    reps = w["B"] // p0["batch"]
    offs0, times0 = rows_to_dof_csr(p0["kp_rows"], p0["dof"], p0["T"])
    E0 = int(offs0[-1])
    offs = np.concatenate([offs0[:-1].astype(np.int64) + r * E0 for r in range(reps)] + [np.array([reps * E0])]).astype(np.int32)
    times = np.tile(times0, reps)
    return p0, reps, offs, times, desc


def bytes_model(p0, reps, offs0, times0):
    dof, n, m, T = p0["dof"], p0["n"], p0["m"], p0["T"]
    sep_r = sep_w = one_r = one_w = 0
    ntile = (T + TILE - 1) // TILE
    for l in range(len(offs0) - 1):
        t = times0[offs0[l]:offs0[l + 1]]
        ncol = 3 if (l % dof) < m else 2
        colb = ncol * n * 8
        E = len(t)
        if E == 0:
            continue
        covered = int(t[-1] - t[0] + 1)
        # entries a tile touches: key-points inside it and the endpoints of the segments that reach into it
        touched = 0
        for k in range(ntile):
            lo, hi = k * TILE, min(T, (k + 1) * TILE) - 1
            a = np.searchsorted(t, lo, "right") - 1
            b = np.searchsorted(t, hi, "left")
            a, b = max(a, 0), min(b, E - 1)
            if t[a] > hi or t[b] < lo:
                continue
            touched += b - a + 1
        sep_r += E * (6 * n + 2) * 8 + E * 3 * n * 8 + touched * colb
        sep_w += E * 3 * n * 8 + E * colb + (covered - E) * colb
        one_r += touched * (2 * colb + 8)
        one_w += covered * colb
    return dict(separate=int(reps * (sep_r + sep_w)), one_pass=int(reps * (one_r + one_w)))


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream); fn(); b.record(stream); b.synchronize()
    return a.elapsed_time(b)


def stage_ms(w, p0, reps, offs, times, nrep, force_sequence):
    if force_sequence:
        os.environ["KPILQR_FD_INTERP"] = "0"
    else:
        os.environ.pop("KPILQR_FD_INTERP", None)
    stream = torch.cuda.Stream(); torch.cuda.set_stream(stream)
    out = {}
    with Engine(p0["dof"], p0["m"], p0["T"], p0["nr"], batch=w["B"], stream=stream.cuda_stream) as e:
        os.environ.pop("KPILQR_FD_INTERP", None)
        assert "fused" not in e.backward_variant
        has = hasattr(e._L, "kpilqr_fd_interpolate")
        e.set_keypoints(offs, times)
        s0 = e.fd_kp_slab(*synth.kp_ordered_payload(p0), pinned=False)
        nb = s0["entries"] * s0["layout"].entry_stride
        slab = dict(slab=np.tile(s0["slab"][:nb], reps), entries=s0["entries"] * reps, layout=s0["layout"])

        def stage():
            if has:
                e.fd_interpolate()
            else:
                e.fd_difference(); e.interpolate()
        ms = []
        for i in range(nrep + 1):
            e.upload_fd_kp(slab, eps=p0["eps"]); e.sync()
            ms.append(timed(stream, stage))
        out["fresh_payload_ms"] = [round(x, 4) for x in ms[1:]]
        out["ms"] = float(np.median(ms[1:]))
        out["form"] = e.last_launch("linearise") if has else "fd_difference+interpolate (library without kpilqr_fd_interpolate)"
        if has and not force_sequence:
            back = [timed(stream, e.fd_interpolate) for _ in range(nrep + 1)][1:]
            out["back_to_back_ms"] = float(np.median(back))
        # a checksum of the first 4096 step records (their [A|B] parts are what the stage wrote): the libraries must agree on it
        L = RecStride(p0["n"], p0["m"])
        nrec = min(4096, w["B"] * p0["T"])
        rec = torch.as_tensor(e.device_array(0, (nrec, L)), device="cuda")[:, :p0["n"] * (p0["n"] + p0["m"])]
        out["checksum"] = float(rec.double().abs().sum().item())
        del rec
    return out


def RecStride(n, m):
    """Doubles from one step record to the next (RecLayout, csrc/common.h)."""
    return (2 * n * n + n * m + n + m * m + m + 15) & ~15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["cfg2", "cfg4", "panda"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = os.environ.get("KPILQR_LIB") or "in-tree"
    lines = []
    for name in args.workloads:
        w = WORKLOADS[name]
        t0 = time.time()
        p0, reps, offs, times, desc = build(w)
        offs0, times0 = rows_to_dof_csr(p0["kp_rows"], p0["dof"], p0["T"])
        row = dict(workload=name, desc=desc, library=lib, batch=w["B"], entries=int(offs[-1]),
                   keypoint_fraction=float(offs[-1]) / (w["B"] * p0["dof"] * p0["T"]), bytes_model=bytes_model(p0, reps, offs0, times0))
        row["stage"] = stage_ms(w, p0, reps, offs, times, args.reps, False)
        if "fd_interpolate" in row["stage"]["form"] or "kp_columns" in row["stage"]["form"]:
            row["stage_KPILQR_FD_INTERP_0"] = stage_ms(w, p0, reps, offs, times, args.reps, True)
            row["one_pass_TBps"] = row["bytes_model"]["one_pass"] / (row["stage"]["ms"] * 1e-3) / 1e12
        else:
            row["separate_TBps"] = row["bytes_model"]["separate"] / (row["stage"]["ms"] * 1e-3) / 1e12
        row["host_seconds"] = round(time.time() - t0, 1)
        lines.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
