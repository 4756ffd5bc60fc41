"""Timing of KPILQR_FLAG_EMBED_SHAPE: a one-tile shape without sweep kernels of its own, run embedded in its carrier shape (the
fused sweeps) against the same build with KPILQR_FLAG_FUSED alone -- the path such a shape takes without the flag (tiled or generic
kernels on step records).

    python tools/embed_timing.py [--T 3000] [--batches 64,1024] [--warmup 5] [--reps 20] [--out profiles/embedded_shapes.txt]

Shapes shape_task(6,6,12) and shape_task(3,2,6), key-points every 5 steps, the key-point ordered payload, the task's constant
residual Jacobian.  Everything is timed with events on the context's stream, in one process on one box:
  iterate    the whole kpilqr_iterate, resident inputs: median [min .. max] of --reps calls after --warmup
  upload     kpilqr_upload_fd_kp from pinned memory: on the embedded context one DMA of the caller's records + k_embed_fd_kp
  gains      kpilqr_download_gains into pinned memory: on the embedded context k_extract_gains (K, k) + two DMAs of the compact
             arrays; beside it the plain download of a context created natively at the CARRIER's shape (the bytes the embedded
             context would move without the extraction), and the ratio of the two
The embedding launches are part of the upload and gains calls, not of iterate.  Their own times, without the copies, come from a
run under `rocprofv3 --kernel-trace --stats` (kernels k_embed_entries, k_embed_rows, k_extract_gains).
16 distinct trajectories are tiled over the batch; the embedded and the plain context are checked against each other (1e-9 of the
largest gain) before anything is timed."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajoptkp_amd import Engine, synth  # noqa: E402
from trajoptkp_amd.engine import rows_to_dof_csr  # noqa: E402

SHAPES = ((6, 6, 12), (3, 2, 6))
DISTINCT = 16


def event_ms(stream, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(); b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def fmt(t):
    return f"{t[0]:9.3f} ms [{t[1]:9.3f} .. {t[2]:9.3f}]"


def tiled_inputs(dof, m, nr, T, B):
    base = synth.make_problem(task=synth.shape_task(dof, m, nr), T=T, batch=min(DISTINCT, B), min_N=5)
    reps = -(-B // base["batch"])
    xp, xm, mode = synth.kp_ordered_payload(base)
    offs, times = rows_to_dof_csr(base["kp_rows"], dof, T)
    E0 = int(offs[-1])
    offs_all = np.concatenate([offs[:-1] + i * E0 for i in range(reps)] + [[reps * E0]]).astype(np.int32)[:B * dof + 1]
    ent = int(offs_all[-1])
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))
    return dict(base=base, offs=offs_all, times=np.tile(times, reps)[:ent], xp=tile(xp)[:ent], xm=tile(xm)[:ent], mode=tile(mode)[:ent],
                r=tile(base["r"])[:B], u_nom=tile(base["u_nom"])[:B])


def run(dof, m, nr, T, B, warmup, reps, lines):
    inp = tiled_inputs(dof, m, nr, T, B)
    base = inp["base"]
    stream = torch.cuda.Stream()
    alphas = np.array([(i / 6.0) ** 2 for i in range(1, 7)])
    out, slab = {}, None
    for embed in (True, False):
        with Engine(dof, m, T, nr, batch=B, stream=stream.cuda_stream, fused=True, embed=embed) as e:
            e.set_keypoints(inp["offs"], inp["times"])
            if slab is None:
                slab = e.fd_kp_slab(inp["xp"], inp["xm"], inp["mode"])
            e.upload_residuals(inp["r"], None, None, base["w_run"], base["w_term"])
            e.upload_residual_jacobians_const(base["rx_const"], None)
            e.upload_nominal(inp["u_nom"], base["ctrl_lim"])
            e.upload_fd_kp(slab, eps=base["eps"])
            e.sync()
            K = e.pinned((B, T, 2 * dof, m)); k = e.pinned((B, T, m))
            import ctypes as C
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            e.iterate(base["lam"], 100, alphas)
            e._ck(e._L.kpilqr_download_gains(e._h, p(K), p(k))); e.sync()
            res = e.results()
            assert not np.any(res["status"]), res["status"]
            t_it = event_ms(stream, lambda: e.iterate(None, 100, None), warmup, reps)
            t_up = event_ms(stream, lambda: e.upload_fd_kp(slab, eps=base["eps"]), 2, reps)
            t_dn = event_ms(stream, lambda: e._ck(e._L.kpilqr_download_gains(e._h, p(K), p(k))), 2, reps)
            out[embed] = dict(K=np.array(K[:DISTINCT]), cost=res["cost_pred"][:DISTINCT], it=t_it, up=t_up, dn=t_dn,
                              variant=e.backward_variant, launch=e.last_launch("backward"),
                              carrier=e.carrier_dims() if embed else None)
    a, b = out[True], out[False]
    err = float(np.max(np.abs(a["K"] - b["K"])) / np.max(np.abs(b["K"])))
    assert err <= 1e-9, err
    cdof, cm = a["carrier"]
    with Engine(cdof, cm, T, nr, batch=B, stream=stream.cuda_stream, fused=True) as e:       # the carrier's own plain download
        import ctypes as C
        K = e.pinned((B, T, 2 * cdof, cm)); k = e.pinned((B, T, cm))
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        t_nat = event_ms(stream, lambda: e._ck(e._L.kpilqr_download_gains(e._h, p(K), p(k))), 2, reps)
    head = f"shape ({dof},{m}) nr={nr} T={T} B={B:4d}"
    lines += [
        f"{head}  embedded in ({cdof},{cm})  {a['launch']}",
        f"    iterate  embedded {fmt(a['it'])} | FUSED alone ({b['variant']}) {fmt(b['it'])} | embedded / plain {a['it'][0] / b['it'][0]:.3f}   (K of the two within {err:.1e})",
        f"    upload   embedded {fmt(a['up'])} (DMA + k_embed_fd_kp) | FUSED alone {fmt(b['up'])} (DMA)",
        f"    gains    embedded {fmt(a['dn'])} (k_extract_gains + DMA, {B * T * (2 * dof + 1) * m * 8 / 1e6:.1f} MB) | carrier's own download "
        f"{fmt(t_nat)} ({B * T * (2 * cdof + 1) * cm * 8 / 1e6:.1f} MB) | embedded / carrier {a['dn'][0] / t_nat[0]:.3f} | FUSED alone {fmt(b['dn'])}",
    ]
    for line in lines[-4:]:
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=3000)
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}; events on the context's stream; median [min .. max] of {a.reps} calls after {a.warmup} warm-up calls; "
             f"key-points every 5 steps, key-point ordered payload, constant residual Jacobian"]
    for dof, m, nr in SHAPES:
        for B in (int(x) for x in a.batches.split(",")):
            run(dof, m, nr, a.T, B, a.warmup, a.reps, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
