"""What the sweeps over a listed subset (kpilqr_backward_partial + kpilqr_forward_linear_partial) cost on the headline shape: Panda
reaching, T = 3000, 1024 distinct seeds (bench.py's generator), the fused sweeps on the key-point ordered payload with the constant
residual Jacobian.

    python tools/partial_sweeps_timing.py [--batch B] [--horizon T] [--reps N] [--out FILE]

The listed backward + forward sweep between two events on the context's stream, after a warm-up, for a SCATTERED 1, 3/4, 1/2, 1/4 and
1/16 of the batch (every list is a random subset, sorted; the list lives in pinned memory and the lambdas are the resident ones, so
the calls do not wait for the stream), against the whole-batch calls (kpilqr_backward + kpilqr_forward_linear) in the same process:
the routes ALTERNATE, the whole-batch route before every other one -- the spread of its runs stands beside each figure.  The column
store is valid throughout (kpilqr_fd_difference once, before the clock): both routes read it, neither differences inside a sweep.
The launch strings say which form each list's length chose."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARES = ((1, 1), (3, 4), (1, 2), (1, 4), (1, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T = a.batch, a.horizon
    import bench
    p = bench.distinct_problem("panda_reaching", T, B, 5, cache=os.environ.get("KPILQR_WORKLOAD_CACHE"))          # (forks: before anything initialises the GPU)
    import torch
    from oracle import oracle as orc
    from trajoptkp_amd import Engine, synth
    alphas = orc.alphas(6)
    stream = torch.cuda.Stream()
    lines = [f"# {torch.cuda.get_device_name(0)}; panda_reaching T={T} B={B} distinct seeds, fused, key-point ordered payload differenced once "
             f"(both routes read the column store), constant r_x; median [min .. max] of {a.reps} event-timed backward + forward sweeps per route, alternating"]
    rng = np.random.default_rng(7)
    with Engine(p["dof"], p["m"], T, p["nr"], batch=B, stream=stream.cuda_stream, fused=True) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=True)
        e.fd_difference()
        e.backward(p["lam"], 100, fetch=False)
        e.forward_linear(alphas, fetch=False); e.sync()
        L, h = e._L, e._h

        def timed(fn):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream); fn(); t1.record(stream); t1.synchronize()
            e.sync()
            return t0.elapsed_time(t1)

        def whole():
            e._ck(L.kpilqr_backward(h, None, 100, None, None))
            e._ck(L.kpilqr_forward_linear(h, None, None, None))

        def listed(traj):
            ptr, cnt = traj.ctypes.data_as(C.c_void_p), len(traj)

            def run():
                e._ck(L.kpilqr_backward_partial(h, cnt, ptr, None, 100, None, None))
                e._ck(L.kpilqr_forward_linear_partial(h, cnt, ptr, None, None, None))
            return run

        routes = []
        for num, den in SHARES:
            cnt = B * num // den
            traj = e.pinned((cnt,), np.int32)
            traj[:] = np.sort(rng.choice(B, cnt, replace=False)).astype(np.int32)
            routes.append((f"listed, a scattered {num}/{den} of the batch ({cnt})", listed(traj), cnt))
        launch = {}
        for _ in range(2):                                                   # warm-up: code objects, every route once
            timed(whole)
            for name, fn, _ in routes:
                timed(fn)
                launch[name] = e.last_launch("backward") + " | " + e.last_launch("forward")
        timed(whole)
        launch_whole = e.last_launch("backward") + " | " + e.last_launch("forward")
        t_base, t_route = [], {name: [] for name, _, _ in routes}
        for _ in range(a.reps):
            for name, fn, _ in routes:
                t_base.append(timed(whole))
                t_route[name].append(timed(fn))
        fmt = lambda t: f"{np.median(t):8.3f} ms [{min(t):8.3f} .. {max(t):8.3f}]"
        lines.append(f"{'whole batch (kpilqr_backward + kpilqr_forward_linear)':52s}: {fmt(t_base)}   over {len(t_base)} runs: the spread every figure below stands beside")
        lines.append(f"{'':52s}  {launch_whole}")
        ref = np.median(t_base)
        for name, _, cnt in routes:
            lines.append(f"{name:52s}: {fmt(t_route[name])}   {np.median(t_route[name]) / ref:5.2f} x the whole batch")
            lines.append(f"{'':52s}  {launch[name]}")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
