"""What kpilqr_iterate_streamed6 with r_x32 / r_u32 costs on the PCIe-inclusive route at the headline shape: Panda reaching, T = 3000,
nr = 14, dense_residuals="smooth" (per-step residual Jacobians: 4.71 MB of r_x and 2.35 MB of r_u per trajectory as FP64), three
chunks, the fused sweeps on a resident key-point ordered payload; the Jacobians up and K, k, cost_pred, delta_J, status down.

    python tools/streamed_residual_jacobians_f32_timing.py [--batches 1024,256] [--horizon T] [--steps N] [--rounds R] [--out FILE]

Per batch size, and per KPILQR_PIPE_COPY setting (unset: uploads by SDMA into the staging buffer; 3: the widening kernel reads the
caller's pinned floats), two cases: the whole batch, and a scattered quarter (every fourth trajectory) with upload_traj = gain_traj =
sweep_traj.  Every case is measured against kpilqr_iterate_streamed5 with the SAME lists and the Jacobians as FP64 -- the call a host
had before -- in the same process and on the same context.  The two legs alternate inside every round; the host clock runs around
`steps` calls and the kpilqr_sync behind them, and the spread over the rounds stands beside every median.
The FP64 leg is fed the widened floats, so both legs compute the same gains: K and k of the two legs are compared bit for bit before
anything is timed.  One trajectory's Jacobians are tiled over the batch: a transfer does not care.  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TASK, MIN_N = "panda_reaching", 5


def build(B, T):
    """the problem of a batch size, built once for both KPILQR_PIPE_COPY settings: one trajectory tiled, its Jacobians kept apart"""
    from trajoptkp_amd import synth
    one = synth.make_problem(task=TASK, T=T, batch=1, min_N=MIN_N, dense_residuals="smooth")
    x32_1, u32_1 = synth.residual_jacobians_f32(one)
    slim = dict(one)
    slim["r_x"], slim["r_u"] = np.zeros((1, 0)), np.zeros((1, 0))  # (the Jacobians are tiled straight into pinned memory)
    p = synth.tile_problem(slim, B)
    return p, x32_1, u32_1, synth.kp_ordered_payload(p)


def run(built, T, nchunks, steps, rounds, pipe_copy, lines):
    from trajoptkp_amd import Engine
    os.environ.pop("KPILQR_PIPE_COPY", None)
    if pipe_copy is not None:
        os.environ["KPILQR_PIPE_COPY"] = pipe_copy                # read when the context is created
    p, x32_1, u32_1, payload = built
    B, n, m, nr = p["batch"], p["n"], p["m"], p["nr"]
    with Engine(p["dof"], m, T, nr, batch=B, fused=True) as e:
        e.set_keypoints_rows(p["kp_rows"])
        e.upload_fd_kp(e.fd_kp_slab(*payload, pinned=False), eps=p["eps"])
        e.upload_residuals(p["r"], None, None, p["w_run"], p["w_term"])
        e.upload_nominal(p["u_nom"], p["ctrl_lim"])
        e.forward_linear((np.arange(1, 7) / 6.0) ** 2, fetch=False)
        x32 = e.pinned((B, T + 1, nr, n), np.float32); x32[:] = x32_1[0]
        u32 = e.pinned((B, T + 1, nr, m), np.float32); u32[:] = u32_1[0]
        x64 = e.pinned((B, T + 1, nr, n)); x64[:] = x32_1[0]        # the widened floats: the FP64 leg computes the same gains
        u64 = e.pinned((B, T + 1, nr, m)); u64[:] = u32_1[0]
        lam = e.pinned(B); lam[:] = p["lam"]
        K = e.pinned((B, T, n, m)); k = e.pinned((B, T, m))
        cost = e.pinned((B, e.n_alpha)); dJ = e.pinned(B); status = e.pinned(B, np.int32)
        per = (T + 1) * nr * (n + m)
        quarter = np.arange(1, B, 4, dtype=np.int32)               # no two listed trajectories are adjacent
        for title, traj in (("whole batch", None), (f"a scattered quarter ({len(quarter)} of {B} trajectories, every fourth) uploaded, swept and brought down", quarter)):
            c = B if traj is None else len(traj)
            kw = dict(eps=p["eps"], lam=lam[:c], K=K[:c], k=k[:c], cost_pred=cost[:c], delta_J=dJ[:c], status=status[:c], nchunks=nchunks)
            if traj is not None:
                kw.update(upload_traj=traj, gain_traj=traj, sweep_traj=traj)
            legs = (("streamed5, FP64 r_x / r_u", lambda: e.iterate_streamed5(r_x=x64[:c], r_u=u64[:c], **kw), c * per * 8),
                    ("streamed6, r_x32 / r_u32", lambda: e.iterate_streamed6(r_x32=x32[:c], r_u32=u32[:c], **kw), c * per * 4))
            got, launch = {}, {}
            for name, fn, _ in legs:                               # warm-up (the staging buffer reserved), and what each leg computes
                K[...] = 0; k[...] = 0
                fn(); fn(); e.sync()
                got[name] = (np.array(K[:c]), np.array(k[:c]), np.array(status[:c]))
                launch[name] = e.last_launch("backward") + " | " + e.last_launch("forward")
            (K5, k5, s5), (K6, k6, s6) = (got[name] for name, _, _ in legs)
            assert np.all(s5 == 0) and np.any(K5 != 0)
            assert np.array_equal(K5, K6) and np.array_equal(k5, k6) and np.array_equal(s5, s6), "the two legs differ"
            times = dict((name, []) for name, _, _ in legs)
            for _ in range(rounds):
                for name, fn, _ in legs:                           # alternating: both legs see the same machine
                    e.sync()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        fn()
                    e.sync()
                    times[name].append(1e3 * (time.perf_counter() - t0) / steps)
            fmt = lambda t: f"{np.median(t):8.2f} ms [{min(t):8.2f} .. {max(t):8.2f}]"
            base = float(np.median(times[legs[0][0]]))
            lines.append(f"B={B}, KPILQR_PIPE_COPY {'unset' if pipe_copy is None else '= ' + pipe_copy}, {title}: K, k, status of the two legs equal bit for bit")
            for name, _, nbytes in legs:
                t = float(np.median(times[name]))
                lines.append(f"  {name:28s} {nbytes / 1e9:6.3f} GB of Jacobians: {fmt(times[name])}  {c / t * 1e3:8.0f} traj-it/s  x{base / t:.3f}")
                lines.append(f"  {'':28s} {launch[name]}")
        del x32, u32, x64, u64, K, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,256")
    ap.add_argument("--horizon", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunks", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("streamed_residual_jacobians_f32_timing: no GPU (nothing is timed on a CPU)")
    lines = [f"# {torch.cuda.get_device_name(0)}; {TASK} T={a.horizon}, dense_residuals=\"smooth\" (one trajectory tiled), fused, resident key-point ordered "
             f"payload, per-step r_x + r_u up and K + k + cost_pred + delta_J + status down, {a.chunks} chunks; ms per iteration, median [min .. max] of "
             f"{a.rounds} rounds of {a.steps} calls and one wait, the two legs alternating"]

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write("\n".join(lines) + "\n")
    for B in (int(b) for b in a.batches.split(",")):
        built = build(B, a.horizon)
        for pipe_copy in (None, "3"):
            run(built, a.horizon, a.chunks, a.steps, a.rounds, pipe_copy, lines)
            print("\n".join(lines[-8:]), flush=True)
            flush()


if __name__ == "__main__":
    main()
