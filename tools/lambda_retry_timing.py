"""What the lambda retry schedule (kpilqr_set_lambda_retry) costs and saves on the headline shape: Panda reaching, T = 3000,
1024 distinct seeds (bench.py's generator), the fused sweeps on the key-point ordered payload with the constant residual Jacobian.

    python tools/lambda_retry_timing.py [--batch B] [--horizon T] [--reps N] [--out FILE]

Whole iterations (kpilqr_iterate: backward + forward) between two events on the context's stream, after a warm-up, the routes
ALTERNATING in one process, (a) before every other one -- the spread of the (a) runs stands beside each figure:
  (a) schedule off, nobody failing                      the iteration of a library without the schedule
  (b) schedule on with max_attempts = 1                 + k_lambda_retry_begin, and nothing else
  (b2) schedule on, nobody failing, one retry allowed   + one k_lambda_retry and one gated-out launch sequence
  (c1) / (c10) schedule on, 1 / every 10th trajectory needing one retry
  (d1) / (d10) the host loop on the inputs of (c): kpilqr_backward, kpilqr_sync, a host pass over status, kpilqr_backward for the
               whole batch, kpilqr_forward_linear
PD checks fail because the running weights are NEGATIVE (w_run = -0.1 |w_run|): at lambda = 0.01 Q_uu + lambda I turns indefinite
some hundred steps into the sweep for most seeds, at lambda = 100 for none (at lambda = 1 about 2 % of 1024 seeds still fail: a first
version of this tool took 1 for the good lambda and timed their retries as "nobody failing").  The tool's schedule is factor 1e4,
max_lambda 1e6: 0.01 -> 100 is ONE retry, and from 100 one more attempt is allowed, which nobody needs.
It also writes the two histograms that price a restart INSIDE the wave: attempts per trajectory, and how deep
into the sweep the first attempt failed, (T - failing step) / T, with every trajectory started at lambda = 0.01."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAM_OK, LAM_FAIL = 100.0, 0.01
SCHED = dict(factor=1e4, max_lambda=1e6, max_attempts=4)


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
    p["w_run"] = -0.1 * np.abs(p["w_run"])
    import torch
    from oracle import oracle as orc
    from trajoptkp_amd import Engine, synth
    alphas = orc.alphas(6)
    stream = torch.cuda.Stream()
    lines = [f"# {torch.cuda.get_device_name(0)}; panda_reaching T={T} B={B} distinct seeds, fused, key-point ordered payload, constant r_x; "
             f"w_run = -0.1 |w_run|; schedule {SCHED}; median [min .. max] of {a.reps} event-timed iterations per route, alternating"]

    def lam_for(every):
        lam = np.full(B, LAM_OK)
        if every:
            lam[::every] = LAM_FAIL
        return lam

    with Engine(p["dof"], p["m"], T, p["nr"], batch=B, stream=stream.cuda_stream, fused=True) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=True)
        e.forward_linear(alphas, fetch=False); e.sync()

        def timed(fn):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream); fn(); t1.record(stream); t1.synchronize()
            e.sync()
            return t0.elapsed_time(t1)

        def device_route(lam, sched):
            def run():
                e.set_lambda_retry(**sched) if sched else e.set_lambda_retry(None)
                e.iterate(lam, 100, alphas)
            return run

        def host_route(lam0):
            def run():
                e.set_lambda_retry(None)
                lam = lam0.copy(); pending = np.ones(B, bool)
                while True:
                    status, _ = e.backward(lam, pd_stride=100)              # (syncs)
                    again = False
                    for b in np.nonzero(pending)[0]:
                        nxt = lam[b] * SCHED["factor"]
                        if status[b] == 0 or nxt > SCHED["max_lambda"]:
                            pending[b] = False
                        else:
                            lam[b] = nxt; again = True
                    if not again:
                        break
                e.forward_linear(alphas, fetch=False)
            return run

        one = np.full(B, LAM_OK); one[B // 2] = LAM_FAIL
        routes = [("(b)   on, max_attempts = 1: no second attempt", device_route(lam_for(0), dict(SCHED, max_attempts=1)), None),
                  ("(b2)  on, nobody failing, one gated-out attempt", device_route(lam_for(0), SCHED), None),
                  ("(c1)  on, 1 trajectory retried once", device_route(one, SCHED), None),
                  ("(c10) on, every 10th trajectory retried once", device_route(lam_for(10), SCHED), None),
                  ("(d1)  host loop, 1 trajectory retried once", host_route(one), None),
                  ("(d10) host loop, every 10th trajectory retried once", host_route(lam_for(10)), None)]
        base = device_route(lam_for(0), None)
        for _ in range(2):                                                   # warm-up: code objects, every route once
            timed(base)
            for _, fn, off in routes:
                timed(fn)
        t_base, t_route = [], {name: [] for name, _, _ in routes}
        for _ in range(a.reps):
            for name, fn, off in routes:
                t_base.append(timed(base))
                t_route[name].append(timed(fn))
        fmt = lambda t: f"{np.median(t):8.3f} ms [{min(t):8.3f} .. {max(t):8.3f}]"
        lines.append(f"(a)   off, nobody failing (lambda = {LAM_OK}): {fmt(t_base)}   over {len(t_base)} runs: the spread every figure below stands beside")
        for name, _, _ in routes:
            ref = np.median(t_base)
            lines.append(f"{name:52s}: {fmt(t_route[name])}   {np.median(t_route[name]) - ref:+8.3f} ms against (a)")
        # histograms: attempts, and the depth of the first failure, everybody started at the failing lambda
        e.set_lambda_retry(None)
        status, _ = e.backward(np.full(B, LAM_FAIL), pd_stride=100)
        failed = status != 0
        depth = (T - status[failed]) / T
        e.set_lambda_retry(**SCHED)
        e.backward(np.full(B, LAM_FAIL), pd_stride=100, fetch=False)
        lam_used, att = e.lambda_retry()
        final = e.results()["status"]
        lines.append(f"everybody at lambda = {LAM_FAIL}: {int(failed.sum())} of {B} fail their first sweep; attempts histogram "
                     f"{dict(zip(*map(lambda x: x.tolist(), np.unique(att, return_counts=True))))}; still failed after the schedule: {int((final != 0).sum())}")
        if failed.any():
            h, edges = np.histogram(depth, bins=10, range=(0.0, 1.0))
            lines.append("depth of the first failure, (T - failing step) / T, share of the failing trajectories per tenth of the sweep: "
                         + " ".join(f"{x:.2f}" for x in h / h.sum()) + f"   (mean {depth.mean():.3f}, min {depth.min():.3f}, max {depth.max():.3f})")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
