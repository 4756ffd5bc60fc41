"""What kpilqr_iterate_streamed5 with sweep_traj costs on the PCIe-inclusive route at the headline shape: Panda reaching, T = 3000,
B = 1024, three chunks, the fused sweeps with the constant residual Jacobian, FP64 key-point columns, r and u_nom up and K, k down
for the LISTED trajectories.

    python tools/streamed_subset_sweeps_timing.py [--batch B] [--horizon T] [--steps N] [--rounds R] [--out FILE]

A scattered 1/32, 1/4, 1/2 and all of the batch is listed, and upload_traj = gain_traj = sweep_traj.  Every share is measured against
kpilqr_iterate_streamed4 with the SAME upload and gain lists in the same process -- the call a host had before: it moves the same
bytes and sweeps every trajectory of every chunk.  The two legs of a share alternate inside every round; the host clock runs around
`steps` calls and the kpilqr_sync behind them, and the spread over the rounds stands beside every median.
The listed trajectories are sent the values and lambdas they already have, so both legs compute the same gains for them: the largest
relative difference is printed (the forms differ with the launch width, so it is rounding, not zero), and the launch strings say
which form each leg's last chunk chose.  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARES = ((1, 32), (1, 4), (1, 2), (1, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunks", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, nchunks = a.horizon, a.chunks
    import torch
    from trajoptkp_amd import Engine, synth
    uniq = min(8, a.batch)
    p = synth.tile_problem(synth.make_problem(task="panda_reaching", T=T, batch=uniq, min_N=5), a.batch // uniq)
    B, n, m = p["batch"], p["n"], p["m"]
    lines = [f"# {torch.cuda.get_device_name(0)}; panda_reaching T={T} B={B} ({uniq} distinct trajectories tiled), fused, constant r_x, FP64 key-point "
             f"columns + r + u_nom up and K + k down for the listed, {nchunks} chunks; ms per iteration, median [min .. max] of {a.rounds} rounds of "
             f"{a.steps} calls and one wait, the legs of a share alternating"]
    with Engine(p["dof"], m, T, p["nr"], batch=B, fused=True) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=True)
        r = e.pinned(p["r"].shape); r[...] = p["r"]
        u_nom = e.pinned(p["u_nom"].shape); u_nom[...] = p["u_nom"]
        lam = e.pinned(B); lam[:] = p["lam"]
        cols = e.kp_columns(*synth.kp_ordered_payload(p), eps=p["eps"])
        E = cols["entries"]
        per = E // B                                         # (a tiled problem with set-interval key-points: the same count for everybody)
        assert per * B == E
        c64 = cols["cols"][:E * 3 * n].reshape(B, per * 3 * n)
        K = e.pinned((B, T, n, m)); k = e.pinned((B, T, m))
        cost = e.pinned((B, e.n_alpha)); dJ = e.pinned(B); status = e.pinned(B, np.int32)
        sc_cols = e.pinned((B, per * 3 * n)); sc_r = e.pinned(r.shape); sc_u = e.pinned(u_nom.shape); sc_lam = e.pinned(B)
        # the whole batch resident, swept once
        e.iterate_streamed3(kp_cols=cols, eps=p["eps"], r=r, u_nom=u_nom, lam=lam, K=K, k=k, nchunks=nchunks)
        e.sync()

        def leg(traj, five):
            c = len(traj)
            kw = dict(kp_cols=dict(cols=sc_cols[:c].reshape(-1), entries=c * per), eps=p["eps"], r=sc_r[:c], u_nom=sc_u[:c], K=K[:c], k=k[:c],
                      nchunks=nchunks, upload_traj=traj, gain_traj=traj)
            if five:
                return lambda: e.iterate_streamed5(lam=sc_lam[:c], cost_pred=cost[:c], delta_J=dJ[:c], status=status[:c], sweep_traj=traj, **kw)
            return lambda: e.iterate_streamed4(lam=lam, cost_pred=cost, delta_J=dJ, status=status, **kw)

        for num, den in SHARES:
            c = max(1, B * num // den)
            traj = np.unique(np.floor(np.arange(c) * (B / c)).astype(np.int32))
            assert len(traj) == c
            sc_cols[:c] = c64[traj]; sc_r[:c] = r[traj]; sc_u[:c] = u_nom[traj]; sc_lam[:c] = lam[traj]      # the caller's own packing: not timed
            four, five = leg(traj, False), leg(traj, True)
            got, launch = {}, {}
            for name, fn in (("streamed4", four), ("streamed5", five)):          # warm-up, and what each leg computes for the listed
                K[...] = 0; k[...] = 0
                fn(); fn(); e.sync()
                got[name] = (np.array(K[:c]), np.array(k[:c]), np.array(status[:c]))
                launch[name] = e.last_launch("backward") + " | " + e.last_launch("forward")
            assert np.any(got["streamed4"][0] != 0) and np.all(got["streamed5"][2] == 0)
            rel = max(float(np.max(np.abs(x - y)) / np.max(np.abs(y))) for x, y in zip(got["streamed5"][:2], got["streamed4"][:2]))
            assert rel < 1e-9, rel
            times = {"streamed4": [], "streamed5": []}
            for _ in range(a.rounds):
                for name, fn in (("streamed4", four), ("streamed5", five)):
                    e.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        fn()
                    e.sync()
                    times[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
            fmt = lambda t: f"{np.median(t):8.2f} ms [{min(t):8.2f} .. {max(t):8.2f}]"
            base = float(np.median(times["streamed4"]))
            lines.append(f"a scattered {num}/{den} of the batch listed ({c}): K, k of the two legs agree to {rel:.1e} relative")
            for name in ("streamed4", "streamed5"):
                t = float(np.median(times[name]))
                lines.append(f"  {name + (', every trajectory swept' if name == 'streamed4' else ', the listed swept'):38s}: {fmt(times[name])}  "
                             f"{c / t * 1e3:9.0f} listed traj-it/s  x{base / t:.3f}")
                lines.append(f"  {'':38s}  {launch[name]}")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
