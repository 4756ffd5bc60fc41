"""Same-process A/B of partial re-linearisation on the bench's per-DoF workload (Panda reaching, T = 3000, B = 1024,
velocity_change(1, 50) lists, key-point ordered payload): python tools/partial_regeneration_timing.py [--batch B] [--fractions ...]
[--samples N] [--out FILE]

A fraction f of the trajectories (a seeded random subset: the regenerating trajectories of a batch are scattered) gets new lists of
other lengths -- trajectory b toggles between the lists of seed b and of seed b + 1 -- and a new payload.  Two routes bring the
context there:
  (a) the whole batch again: kpilqr_set_keypoints + kpilqr_upload_fd_kp of the whole pinned slab (what the batch shim did before)
  (b) kpilqr_update_keypoints + kpilqr_upload_fd_kp_partial: the subset's lists and records; the others' records move on the device
Both run on ONE fused context in one process and alternate (a b b a ...: each toggles the subset's lists, so that both see both
directions); one warm-up round, then --samples (5) timed calls each; host clock from the first call to the completion of the
context's stream; median and min .. max.  The pinned slabs are sized for the larger layout and hold the first layout's records:
the routes are timed, not iterated on (tests/test_gpu_partial_regeneration.py holds their results bit for bit).

Per fraction also, from calls of their own:
  relocation   kpilqr_update_keypoints under HIP events on the context's stream with the payload resident, minus the same call
               after kpilqr_set_keypoints has dropped the payload (lists merged, segment map built, nothing to carry): the two copy
               kernels' share, and the GB/s of its bytes (kept records read once and written once)
  gains        kpilqr_download_gains (whole batch) against kpilqr_download_gains_partial (the subset) into pinned memory, HIP events
Byte model: (b) = f x (a) + one HBM-rate pass over the kept records.  Prints one JSON line per fraction and a table; --out appends."""
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

ALPHAS = np.array([(i / 6.0) ** 2 for i in range(1, 7)])


def csr_of(seeds, dof, offs0, times0):
    """Per-DoF CSR of trajectories that carry the lists of the given seeds of the 8 built ones."""
    lens = np.diff(offs0).reshape(-1, dof)
    blocks = [times0[offs0[s * dof]:offs0[(s + 1) * dof]] for s in range(len(lens))]
    offs = np.concatenate([[0], np.cumsum(lens[seeds].ravel())]).astype(np.int32)
    times = np.concatenate([blocks[s] for s in seeds]) if len(seeds) else np.zeros(0, np.int32)
    return offs, times.astype(np.int32)


def wall(e, fn):
    e.sync()
    t0 = time.perf_counter()
    fn()
    e.sync()
    return (time.perf_counter() - t0) * 1e3


def events(stream, e, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e.sync()
    a.record(stream); fn(); b.record(stream); b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(np.min(ms)), 3), max=round(float(np.max(ms)), 3), n=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--T", type=int, default=3000)
    ap.add_argument("--fractions", nargs="*", type=float, default=[1 / 16, 1 / 4, 1 / 2, 1.0])
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, T, N = args.batch, args.T, args.samples
    stream = torch.cuda.Stream(); torch.cuda.set_stream(stream)
    _, p0, desc = bench.build_problem("reach_velocity_change", 8, T, 1, "panda_reaching", distinct=False)
    dof, n, m, uniq = p0["dof"], p0["n"], p0["m"], p0["batch"]
    offs0, times0 = rows_to_dof_csr(p0["kp_rows"], dof, T)
    xp, xm, mode = synth.kp_ordered_payload(p0)
    base = np.arange(B) % uniq
    rows = []
    with Engine(dof, m, T, p0["nr"], batch=B, stream=stream.cuda_stream, fused=True) as e:
        stride = (6 * n + 2) * 8
        s0 = e.fd_kp_slab(xp, xm, mode, pinned=False)["slab"][:int(offs0[-1]) * stride]
        per_seed = [s0[int(offs0[s * dof]) * stride:int(offs0[(s + 1) * dof]) * stride] for s in range(uniq)]
        o_all = {0: csr_of(base, dof, offs0, times0), 1: csr_of((base + 1) % uniq, dof, offs0, times0)}      # nobody / everybody toggled
        cap = max(int(o_all[0][0][-1]), int(o_all[1][0][-1])) + B * dof * 64
        full = e.pinned(cap * stride, np.uint8)                    # the whole batch's records (first layout)
        part = e.pinned(cap * stride, np.uint8)                    # the subset's, back to back
        at = 0
        for b in range(B):
            rec = per_seed[base[b]]
            full[at:at + len(rec)] = rec; at += len(rec)
        part[:at] = full[:at]
        K = e.pinned((B, T, n, m)); k = e.pinned((B, T, m))
        arr = {key: np.tile(p0[key][:uniq], (B // uniq + 1,) + (1,) * (p0[key].ndim - 1))[:B] for key in ("r", "u_nom")}
        e.set_keypoints(*o_all[0])
        e.upload_residuals(arr["r"], None, None, p0["w_run"], p0["w_term"])
        e.upload_residual_jacobians_const(p0["rx_const"], None)
        e.upload_nominal(arr["u_nom"], p0["ctrl_lim"])
        e.upload_fd_kp(dict(slab=full, entries=int(o_all[0][0][-1])), eps=p0["eps"])
        e.iterate(p0["lam"], 100, ALPHAS); e.sync()
        assert np.all(e.results()["status"] == 0)
        rng = np.random.default_rng(5)
        for f in args.fractions:
            cnt = max(1, int(round(f * B)))
            traj = np.sort(rng.choice(B, cnt, replace=False)).astype(np.int32)
            listed = np.zeros(B, bool); listed[traj] = True
            state = {v: np.where(listed, (base + v) % uniq, base) for v in (0, 1)}      # the seeds every trajectory carries
            whole = {v: csr_of(state[v], dof, offs0, times0) for v in (0, 1)}
            sub = {v: csr_of(state[v][traj], dof, offs0, times0) for v in (0, 1)}

            def route_a(v):
                e.set_keypoints(*whole[v])
                e.upload_fd_kp(dict(slab=full, entries=int(whole[v][0][-1])), eps=p0["eps"])

            def route_b(v):
                e.update_keypoints(traj, *sub[v])
                e.upload_fd_kp_partial(traj, dict(slab=part, entries=int(sub[v][0][-1])), eps=p0["eps"])

            route_a(0); e.sync()
            ms = {"a": [], "b": []}
            v, i = 0, 0
            while min(len(ms["a"]), len(ms["b"])) < N + 2:           # a b b a a b b a ...; the first round of each is warm-up
                name = "ab"[((i + 1) // 2) % 2]
                v ^= 1
                ms[name].append(wall(e, (lambda: route_a(v)) if name == "a" else (lambda: route_b(v))))
                i += 1
            row = dict(batch=B, T=T, desc=desc, fraction=f, listed=cnt, entries=int(whole[0][0][-1]),
                       whole_bytes=int(whole[0][0][-1]) * stride, partial_bytes=int(sub[0][0][-1]) * stride,
                       route_a_ms=stats(ms["a"][2:2 + N]), route_b_ms=stats(ms["b"][2:2 + N]))
            # the relocation's share of kpilqr_update_keypoints: with the payload resident, and with nothing to carry
            carry, bare = [], []
            for j in range(N + 1):
                v ^= 1
                e.upload_fd_kp(dict(slab=full, entries=int(whole[v ^ 1][0][-1])), eps=p0["eps"])
                carry.append(events(stream, e, lambda: e.update_keypoints(traj, *sub[v])))
                v ^= 1
                e.set_keypoints(*whole[v ^ 1])                       # (drops the payload)
                bare.append(events(stream, e, lambda: e.update_keypoints(traj, *sub[v])))
            kept = (int(whole[0][0][-1]) - int(sub[0][0][-1])) * stride
            reloc = float(np.median(carry[1:]) - np.median(bare[1:]))
            row.update(update_carry_ms=stats(carry[1:]), update_bare_ms=stats(bare[1:]), relocation_ms=round(reloc, 3), kept_bytes=kept,
                       relocation_GBps=round(2 * kept / max(reloc, 1e-6) / 1e6, 1) if kept else None)
            e.set_keypoints(*whole[0])
            e.upload_fd_kp(dict(slab=full, entries=int(whole[0][0][-1])), eps=p0["eps"])
            # gains: the whole batch against the subset
            g_all, g_sub = [], []
            for j in range(N + 1):
                g_all.append(events(stream, e, lambda: e._ck(e._L.kpilqr_download_gains(e._h, K.ctypes.data, k.ctypes.data))))
                g_sub.append(events(stream, e, lambda: e._ck(e._L.kpilqr_download_gains_partial(e._h, cnt, traj.ctypes.data, K.ctypes.data, k.ctypes.data))))
            row.update(gains_whole_ms=stats(g_all[1:]), gains_partial_ms=stats(g_sub[1:]), gain_bytes_whole=int(K.nbytes + k.nbytes),
                       gain_bytes_partial=int((K.nbytes + k.nbytes) // B * cnt))
            a, b = row["route_a_ms"]["median"], row["route_b_ms"]["median"]
            row["b_over_a"] = round(b / a, 4)
            row["model_b_ms"] = round(f * a + max(reloc, 0.0), 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    box = f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}"
    out = [f"box: {box}; {desc}; B = {B}, T = {T}; (a) set_keypoints + upload_fd_kp | (b) update_keypoints + upload_fd_kp_partial; ms, median (min..max) of {N}",
           "f       listed  (a) whole batch            (b) partial                b/a     f*a+reloc  relocation ms (GB/s)   update carry / bare   gains whole / partial ms   MB up a / b"]
    for r in rows:
        a, b = r["route_a_ms"], r["route_b_ms"]
        out.append(f"{r['fraction']:<7.4f} {r['listed']:<6}  {a['median']:8.2f} ({a['min']:.2f}..{a['max']:.2f})   {b['median']:8.2f} ({b['min']:.2f}..{b['max']:.2f})   "
                   f"{r['b_over_a']:.3f}   {r['model_b_ms']:8.2f}   {r['relocation_ms']:7.3f} ({r['relocation_GBps']})   "
                   f"{r['update_carry_ms']['median']:.3f} / {r['update_bare_ms']['median']:.3f}   "
                   f"{r['gains_whole_ms']['median']:.2f} / {r['gains_partial_ms']['median']:.2f}   {r['whole_bytes'] / 1e6:.0f} / {r['partial_bytes'] / 1e6:.0f}")
    text = "\n".join(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
