"""Same-process A/B of KPILQR_FLAG_UNION_KEYPOINTS on the bench's two per-DoF workloads (Panda reaching, T = 3000, key-point ordered
payload, constant residual Jacobian): python tools/union_keypoints_timing.py [--kinds ...] [--batches ...] [--reps N] [--out FILE]

  reach_velocity_change   velocity_change(1, 50), reaching.yaml's own key-point method
  reach_adaptive_jerk     adaptive_jerk(1, 50)
  batches                 1024, 512, 256 and one trajectory (bench.py's builders, imported; 8 distinct seeds tiled as BYTES)

Two contexts live side by side on one stream, flag off and flag on.  Every timed iteration starts from a payload that has just been
uploaded (outside the timed region) -- the state of a real iteration, in which both routes difference the payload -- and the two
contexts ALTERNATE, so that clock and thermal drift hit both alike.  HIP events on the contexts' stream; warm-up, then --reps timed
iterations each (default 21); median and the min .. max spread are reported.  The flag-off legs are the parent commit's kernels,
unchanged: they are the baseline of the comparison.

Per case, flag on, from further repetitions of their own:
  union build     wall clock of the first kpilqr_get_union_keypoints size query behind kpilqr_set_keypoints (count kernel, the
                  read-back and wait, the build kernel): once per key-point change
  differencing    kpilqr_fd_difference on the fresh payload (k_fd_kp_difference without the slope store)
  expansion       (first kpilqr_backward behind it: expansion + sweep) - (second kpilqr_backward: the sweep alone), and the GB/s of
                  its own bytes: per union entry 3n doubles written and 4 + 4 bytes of indices read, per own-list entry 3n doubles read
                  (every column is read from memory once, its second reader hits the cache) and its time
  backward / forward sweep, whole iteration, union fraction sum |U_b| / (B T), bytes of kpcu and of kpc
Prints one JSON line per case and, with --out, appends them and a table to FILE."""
import argparse
import ctypes as C
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

ALPHAS = np.array([(i / 6.0) ** 2 for i in range(1, 7)])


def build(kind, T):
    """The workload's 8 distinct trajectories (bench.build_problem's) with their CSR and key-point ordered payload."""
    _, p0, desc = bench.build_problem(kind, 8, T, 1, "panda_reaching", distinct=False)
    offs0, times0 = rows_to_dof_csr(p0["kp_rows"], p0["dof"], T)
    return p0, offs0, times0, synth.kp_ordered_payload(p0), desc


def tiled(p0, offs0, times0, B):
    """Key-point CSR and per-trajectory arrays of B trajectories: the first min(B, 8) seeds, repeated."""
    dof, uniq = p0["dof"], min(B, p0["batch"])
    E0 = int(offs0[uniq * dof])
    reps = B // uniq
    offs = np.concatenate([offs0[:uniq * dof].astype(np.int64) + r * E0 for r in range(reps)] + [np.array([reps * E0])]).astype(np.int32)
    times = np.tile(times0[:E0], reps)
    arr = {k: np.tile(p0[k][:uniq], (reps,) + (1,) * (p0[k].ndim - 1)) for k in ("r", "u_nom")}
    return uniq, reps, E0, offs, times, arr


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream); fn(); b.record(stream); b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return dict(median=round(float(np.median(ms)), 4), min=round(float(np.min(ms)), 4), max=round(float(np.max(ms)), 4), n=len(ms))


def case(kind, B, T, built, nrep, stream):
    p0, offs0, times0, (xp, xm, mode), desc = built
    dof, n, m = p0["dof"], p0["n"], p0["m"]
    uniq, reps, E0, offs, times, arr = tiled(p0, offs0, times0, B)
    row = dict(kind=kind, batch=B, T=T, desc=desc, entries=int(offs[-1]))
    eng, slabs = {}, {}
    try:
        for flag in (False, True):
            e = eng[flag] = Engine(dof, m, T, p0["nr"], batch=B, stream=stream.cuda_stream, fused=True, union_keypoints=flag)
            e.set_keypoints(offs, times)
            if flag:
                e.sync()
                off_u = np.zeros(B + 1, np.int32)
                t0 = time.perf_counter()
                total = e._ck(e._L.kpilqr_get_union_keypoints(e._h, off_u.ctypes.data_as(C.c_void_p), None, 0))
                row["union_build_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
                row["union_fraction"] = total / (B * T)
                row["list_fraction"] = float(offs[-1]) / (B * dof * T)
                row["kpcu_bytes"] = int(dof * total * 3 * n * 8)
                row["kpc_bytes"] = int(offs[-1]) * 3 * n * 8
            s0 = e.fd_kp_slab(xp[:E0], xm[:E0], mode[:E0], pinned=False)
            nb = E0 * s0["layout"].entry_stride
            slabs[flag] = dict(slab=np.tile(s0["slab"][:nb], reps), entries=E0 * reps, layout=s0["layout"])
            e.upload_residuals(arr["r"], None, None, p0["w_run"], p0["w_term"])
            e.upload_residual_jacobians_const(p0["rx_const"], None)
            e.upload_nominal(arr["u_nom"], p0["ctrl_lim"])
            e.upload_fd_kp(slabs[flag], eps=p0["eps"])
            e.iterate(p0["lam"], 100, ALPHAS)                       # lambdas and alphas resident from here on
            e.sync()

        def fresh(flag):
            eng[flag].upload_fd_kp(slabs[flag], eps=p0["eps"]); eng[flag].sync()

        it = {False: [], True: []}
        for i in range(nrep + 2):                                   # two warm-up rounds, then flag off and flag on alternated
            for flag in (False, True):
                fresh(flag)
                ms = timed(stream, lambda: eng[flag].iterate(None, 100, None))
                if i >= 2:
                    it[flag].append(ms)
        for flag in (False, True):
            e = eng[flag]
            key = "on" if flag else "off"
            row[f"iteration_{key}_ms"] = stats(it[flag])
            row[f"launched_{key}"] = e.last_launch("backward") + " | " + e.last_launch("forward")
            parts = dict(diff=[], bwd_first=[], bwd=[], fwd=[])
            for i in range(max(5, nrep // 3) + 1):
                fresh(flag)
                if flag:
                    parts["diff"].append(timed(stream, e.fd_difference))
                parts["bwd_first"].append(timed(stream, lambda: e.backward(None, 100, fetch=False)))
                parts["fwd"].append(timed(stream, lambda: e.forward_linear(None, fetch=False)))
                if flag:
                    parts["bwd"].append(timed(stream, lambda: e.backward(None, 100, fetch=False)))
            med = {k: float(np.median(v[1:])) for k, v in parts.items() if v}
            if flag:
                row["differencing_ms"] = round(med["diff"], 4)
                row["expansion_ms"] = round(med["bwd_first"] - med["bwd"], 4)
                nbytes = row["kpcu_bytes"] + dof * total * 8 + row["kpc_bytes"] + int(offs[-1]) * 4
                row["expansion_bytes"] = nbytes
                row["expansion_GBps"] = round(nbytes / max(row["expansion_ms"], 1e-6) / 1e6, 1)
                row["backward_on_ms"] = round(med["bwd"], 4)
                row["forward_on_ms"] = round(med["fwd"], 4)
            else:
                row["backward_off_ms"] = round(med["bwd_first"], 4)          # (the launch sequence differences per-DoF lists itself)
                row["forward_off_ms"] = round(med["fwd"], 4)
            st = e.results()["status"]
            assert np.all(st == 0), st
        K = {flag: eng[flag].gains()[0] for flag in eng}
        row["K_on_vs_off"] = float(np.max(np.abs(K[True] - K[False])) / np.max(np.abs(K[False])))
        off, on = row["iteration_off_ms"]["median"], row["iteration_on_ms"]["median"]
        row["on_over_off"] = round(on / off, 4)
        row["verdict"] = ("flag on faster by more than 5 %" if on < 0.95 * off else
                          "flag on SLOWER by more than 5 %" if on > 1.05 * off else "within 5 %: no difference this protocol can claim")
    finally:
        for e in eng.values():
            e.close()
    return row


def table(rows):
    out = ["kind                   B     off ms (min..max)         on ms (min..max)          on/off  build   diff    expand (GB/s)    bwd off/on      fwd off/on     |U|/T   kpcu MB  kpc MB"]
    for r in rows:
        a, b = r["iteration_off_ms"], r["iteration_on_ms"]
        out.append(f"{r['kind']:<22} {r['batch']:<5} {a['median']:7.3f} ({a['min']:.3f}..{a['max']:.3f})   {b['median']:7.3f} ({b['min']:.3f}..{b['max']:.3f})   "
                   f"{r['on_over_off']:.3f}  {r['union_build_ms']:6.3f}  {r['differencing_ms']:6.3f}  {r['expansion_ms']:6.3f} ({r['expansion_GBps']:7.1f})  "
                   f"{r['backward_off_ms']:6.3f}/{r['backward_on_ms']:6.3f}  {r['forward_off_ms']:6.3f}/{r['forward_on_ms']:6.3f}  "
                   f"{r['union_fraction']:.3f}  {r['kpcu_bytes'] / 1e6:8.1f} {r['kpc_bytes'] / 1e6:7.1f}   {r['verdict']}")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", nargs="*", default=["reach_velocity_change", "reach_adaptive_jerk"])
    ap.add_argument("--batches", nargs="*", type=int, default=[1024, 512, 256, 1])
    ap.add_argument("--T", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.Stream(); torch.cuda.set_stream(stream)
    rows = []
    for kind in args.kinds:
        built = build(kind, args.T)
        for B in args.batches:
            row = case(kind, B, args.T, built, args.reps, stream)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
    box = f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}"
    text = f"box: {box}\n" + table(rows)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
