"""What kpilqr_iterate_streamed4 with upload_traj saves on the PCIe-inclusive route: Panda reaching, T = 3000, three chunks, FP64
key-point columns, r and u_nom uploaded every iteration, K and k downloaded for everybody.  A fraction f of the batch is listed, once
as a contiguous range and once scattered evenly over the batch; the baseline is kpilqr_iterate_streamed3 with whole inputs in the same
process.  The legs alternate inside every round and the spread over the rounds is printed (profiles/streamed_subset_uploads.txt).

    python tools/streamed_subset_timing.py [batch=1024] [steps=5] [rounds=3] [T=3000] [k32=0]

The listed trajectories get the values they already have, so every leg must reproduce the baseline's K bit for bit: that is asserted
before anything is timed.  Needs a GPU."""
import sys
import time

import numpy as np

from trajoptkp_amd import Engine, synth

FRACTIONS = (1.0, 0.5, 0.25, 0.1)


def lists_for(B, f):
    count = max(1, int(round(B * f)))
    contiguous = np.arange(count, dtype=np.int32)
    scattered = np.unique(np.floor(np.arange(count) * (B / count)).astype(np.int32))
    assert len(scattered) == count
    return contiguous, scattered


def measure(B=1024, steps=5, rounds=3, T=3000, k32=0, nchunks=3, quiet=False):
    uniq = min(8, B)
    p = synth.tile_problem(synth.make_problem(task="panda_reaching", T=T, batch=uniq, min_N=5), B // uniq)
    B = p["batch"]
    with Engine(p["dof"], p["m"], T, p["nr"], batch=B, fused=True) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=True)
        n = p["n"]
        r = e.pinned(p["r"].shape); r[...] = p["r"]
        u_nom = e.pinned(p["u_nom"].shape); u_nom[...] = p["u_nom"]
        lam = e.pinned(B); lam[:] = p["lam"]
        cols = e.kp_columns(*synth.kp_ordered_payload(p), eps=p["eps"])
        E = cols["entries"]
        per = E // B                                         # (a tiled problem with set-interval key-points: the same count for everybody)
        assert per * B == E
        c64 = cols["cols"][:E * 3 * n].reshape(B, per * 3 * n)
        K = e.pinned((B, T, n, p["m"])); k = e.pinned((B, T, p["m"]))
        K32 = e.pinned(K.shape, np.float32) if k32 else None
        down = dict(K32=K32, k=k) if k32 else dict(K=K, k=k)
        half = (B + 1) // 2
        sc_cols = e.pinned((half, per * 3 * n)); sc_r = e.pinned((half,) + r.shape[1:]); sc_u = e.pinned((half,) + u_nom.shape[1:])

        def whole():
            e.iterate_streamed3(kp_cols=cols, eps=p["eps"], r=r, u_nom=u_nom, lam=lam, nchunks=nchunks, **down)

        def listed(traj, contiguous):
            c = len(traj)
            src = (c64, r, u_nom) if contiguous else (sc_cols, sc_r, sc_u)       # a contiguous list from 0: the compact arrays are prefixes
            e.iterate_streamed4(kp_cols=dict(cols=src[0][:c].reshape(-1), entries=c * per), eps=p["eps"], r=src[1][:c], u_nom=src[2][:c], lam=lam,
                                nchunks=nchunks, upload_traj=traj, **down)

        legs = [("streamed3, whole inputs", None, True, 1.0)]
        for f in FRACTIONS:
            cont, scat = lists_for(B, f)
            legs.append((f"streamed4 f={f:<4} contiguous", cont, True, f))
            if f < 1.0:
                legs.append((f"streamed4 f={f:<4} scattered", scat, False, f))

        def run(leg):
            _, traj, contiguous, _ = leg
            if traj is None:
                whole()
            else:
                listed(traj, contiguous)

        def prepare(leg):
            _, traj, contiguous, _ = leg
            if traj is not None and not contiguous:
                c = len(traj)
                sc_cols[:c] = c64[traj]; sc_r[:c] = r[traj]; sc_u[:c] = u_nom[traj]

        # correctness first: every leg gives the baseline's bits
        whole(); e.sync()
        K0 = np.array(K32 if k32 else K); k0 = np.array(k)
        assert np.any(K0 != 0)
        for leg in legs[1:]:
            (K32 if k32 else K)[...] = 0; k[...] = 0
            prepare(leg); run(leg); run(leg); e.sync()
            assert np.array_equal(K32 if k32 else K, K0) and np.array_equal(k, k0), leg[0]
        times = [[] for _ in legs]
        for _ in range(rounds):
            for i, leg in enumerate(legs):
                prepare(leg)                                 # the gather of a scattered list is the caller's own packing: not timed
                e.sync()
                t0 = time.perf_counter()
                for _ in range(steps):
                    run(leg)
                e.sync()
                times[i].append((time.perf_counter() - t0) / steps)
    up_traj = (per * 3 * n * 8 + r[0].nbytes + u_nom[0].nbytes) / 1e6
    dn_traj = ((K32[0].nbytes if k32 else K[0].nbytes) + k[0].nbytes) / 1e6
    base = float(np.median(times[0]))
    rows = []
    for (label, traj, _, f), ts in zip(legs, times):
        dt = float(np.median(ts))
        rows.append(dict(leg=label, f=f, ms_per_iteration=1e3 * dt, ms_rounds=[round(1e3 * t, 2) for t in ts], traj_it_per_s=B / dt,
                         h2d_MB_per_traj=f * up_traj, d2h_MB_per_traj=dn_traj, rate_vs_whole=base / dt))
        if not quiet:
            x = rows[-1]
            print(f"B={B} T={T} {label:32s}: {x['ms_per_iteration']:8.2f} ms (rounds {x['ms_rounds']}) = {x['traj_it_per_s']:9.1f} traj-it/s  "
                  f"x{x['rate_vs_whole']:.3f}  (H2D {x['h2d_MB_per_traj']:.3f} MB + D2H {x['d2h_MB_per_traj']:.3f} MB per trajectory of the batch)", flush=True)
    return dict(batch=B, T=T, steps=steps, rounds=rounds, nchunks=nchunks, k32=bool(k32), rows=rows)


if __name__ == "__main__":
    measure(*[int(x) for x in sys.argv[1:]])
