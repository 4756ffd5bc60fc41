"""PCIe-inclusive iteration rate: every iteration re-uploads the FD payload and the residuals
(+ Jacobians) from PINNED host memory and downloads K, k, as a host that re-linearises every iteration does.
Not the bench metric (bench.py keeps inputs resident; it reports these figures in `pcie_inclusive`).

  python tools/pcie_inclusive.py [batch] [steps]

Forms: "serial"  = kpilqr_upload_fd + kpilqr_upload_residuals + kpilqr_iterate + kpilqr_download_gains + sync per iteration
       "chunks=N" = kpilqr_iterate_streamed over N trajectory chunks (H2D | kernels | D2H overlapped; the FD payload goes up
       key-point ordered, kpilqr_fd_kp_layout), one sync at the end
       of the timed loop ("pipelined") or after every iteration ("per-iteration sync").

  python tools/pcie_inclusive.py gains [batch] [steps] [rounds]

The gain downloads of the chunk pipeline (profiles/streamed_gains.txt): Panda reaching, T = 3000, constant residual Jacobian,
key-point ordered payload, three chunks, pipelined; four legs alternating in one process --
  1 FP64 K through kpilqr_iterate_streamed (the reference of every ratio)      2 K32, whole batch (kpilqr_iterate_streamed2)
  3 K32 of a scattered half of the batch                                         4 FP64 K of the same half
With KPILQR_LIB naming a library without kpilqr_iterate_streamed2 (a build of an earlier commit) leg 1 alone is timed.

  python tools/pcie_inclusive.py columns [batch] [steps] [rounds]

The key-point columns of a host that differences itself, through the chunk pipeline (profiles/streamed_columns_f32.txt): the same
workload, residuals and nominal controls uploaded every iteration, three chunks, pipelined; legs alternating in one process --
  1 FP64 columns through kpilqr_iterate_streamed (kp_cols; the reference of every ratio)
  2 FP32 columns through kpilqr_iterate_streamed3        3 FP32 columns and K32
  0 the key-point ordered x+ / x- payload through kpilqr_iterate_streamed, for scale (what bench.py's pcie_inclusive measures)
With KPILQR_LIB naming a library without kpilqr_iterate_streamed3, legs 0 and 1 alone are timed.
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from trajoptkp_amd import Engine, synth   # noqa: E402


def measure(B=256, steps=5, T=3000, task="panda_reaching", chunk_list=(4, 8, 16), quiet=False):
    uniq = min(8, B)
    p0 = synth.make_problem(task=task, T=T, batch=uniq, min_N=5)
    p = synth.tile_problem(p0, B // uniq)
    B = p["batch"]
    out = {"batch": B, "T": T, "task": task, "steps": steps}
    with Engine(p["dof"], p["m"], T, p["nr"], batch=B, fused=True) as e:
        synth.upload(e, p)
        alphas = np.array([(i / 6.0) ** 2 for i in range(1, 7)])
        e.iterate(p["lam"], 100, alphas); e.sync()
        K0, k0 = e.gains()
        pin = {}
        for name in ("r", "r_x", "r_u", "u_nom", "xplus", "xminus", "xnom"):
            pin[name] = e.pinned(p[name].shape); pin[name][...] = p[name]
        ints = {}
        for name, dt in (("job_b", np.int32), ("job_t", np.int32), ("job_col", np.int32), ("job_nom", np.int32), ("job_mode", np.uint8)):
            ints[name] = e.pinned(p[name].shape, dt); ints[name][...] = p[name]
        lam = e.pinned(B); lam[:] = p["lam"]
        K = e.pinned(K0.shape); k = e.pinned(k0.shape)
        # the chunk pipeline ships the key-point ordered payload (no job lists, no nominal rows; the fused sweeps read it
        # directly); the serial form keeps round 1's call sequence with the job arrays
        kp_payload = synth.kp_ordered_payload(p)
        slab = e.fd_kp_slab(*kp_payload)
        fd_bytes = slab["layout"].bytes
        # ... or the key-point columns a host has differenced itself (kpilqr_upload_kp_columns): 3n doubles per entry
        cols = e.kp_columns(*kp_payload, eps=p["eps"])
        col_bytes = cols["entries"] * 3 * p["n"] * 8
        res_bytes = {True: pin["r"].nbytes + pin["r_x"].nbytes + pin["r_u"].nbytes, False: pin["r"].nbytes}
        dn_bytes = K.nbytes + k.nbytes
        from trajoptkp_amd.engine import _ptr

        def serial(full):
            e.upload_fd(ints["job_b"], ints["job_t"], ints["job_col"], ints["job_mode"], pin["xplus"], pin["xminus"],
                        job_nom=ints["job_nom"], xnom=pin["xnom"], eps=p["eps"])
            if full:
                e.upload_residuals(pin["r"], pin["r_x"], pin["r_u"])
            else:
                e.upload_residuals(pin["r"])
            e.iterate(lam)
            e._ck(e._L.kpilqr_download_gains(e._h, _ptr(K), _ptr(k)))
            e.sync()

        def streamed(full, nchunks, sync_each, columns=False):
            kw = dict(r=pin["r"], r_x=pin["r_x"], r_u=pin["r_u"]) if full else dict(r=pin["r"])
            kw.update(dict(kp_cols=cols) if columns else dict(fd_kp=slab))
            e.iterate_streamed(eps=p["eps"], lam=lam, K=K, k=k, nchunks=nchunks, **kw)
            if sync_each:
                e.sync()

        def timed(fn, *a):
            fn(*a); fn(*a); e.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn(*a)
            e.sync()
            return (time.perf_counter() - t0) / steps

        rows = []
        for full in (True, False):
            up = fd_bytes + res_bytes[full]
            label = "full payload" if full else "resident Jacobians"
            dt = timed(serial, full)
            rows.append((label, "serial", dt, up))
            for nc in chunk_list:
                for sync_each in (True, False):
                    K[...] = 0
                    dt = timed(streamed, full, nc, sync_each)
                    assert np.array_equal(K, K0) and np.array_equal(k, k0), "streamed K differs from the staged path"
                    rows.append((label, f"chunks={nc} " + ("per-iteration sync" if sync_each else "pipelined"), dt, up))
        # the host-differenced columns as the payload (pipelined form, every chunk count)
        for full in (True, False):
            for nc in chunk_list:
                K[...] = 0
                dt = timed(streamed, full, nc, False, True)
                assert np.array_equal(K, K0) and np.array_equal(k, k0), "streamed K differs from the staged path (key-point columns)"
                rows.append(("columns + " + ("full residual payload" if full else "resident Jacobians"), f"chunks={nc} pipelined", dt,
                             col_bytes + res_bytes[full]))
        e.iterate(lam); e.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            e.iterate(lam)
        e.sync()
        dt_res = (time.perf_counter() - t0) / steps
        # Reaching has ONE residual Jacobian (Reaching.cpp:43-54): a host with analytic residuals uploads it once
        # (kpilqr_upload_residual_jacobians_const) and ships, per iteration, the FD payload + the residuals -- the FULL payload
        # of such a task.  Same H2D bytes as "resident Jacobians"; the sweeps no longer read r_x from HBM either.
        if p.get("rx_const") is not None:
            e.upload_residual_jacobians_const(p["rx_const"], None)
            for columns, label in ((False, "constant Jacobians (full payload of a task with analytic residuals)"),
                                   (True, "columns + constant Jacobians")):
                for nc in chunk_list:
                    K[...] = 0
                    dt = timed(streamed, False, nc, False, columns)
                    # (the :rxc sweeps form l_x from the resident r_x' W r_x tile in another accumulation order: K in the same bits, k to 1e-12)
                    assert np.array_equal(K, K0) and np.max(np.abs(k - k0)) <= 1e-12 * np.max(np.abs(k0)), "streamed K differs from the staged path (constant Jacobians)"
                    rows.append((label, f"chunks={nc} pipelined", dt, (col_bytes if columns else fd_bytes) + res_bytes[False]))
            e.iterate(lam); e.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                e.iterate(lam)
            e.sync()
            out["resident_constant_jacobians_traj_it_per_s"] = B / ((time.perf_counter() - t0) / steps)
    out["resident_traj_it_per_s"] = B / dt_res
    out["rows"] = [dict(payload=a, form=b, ms_per_iteration=1e3 * dt, traj_it_per_s=B / dt, h2d_GB=up / 1e9, d2h_GB=dn_bytes / 1e9,
                        link_GBps=(up + dn_bytes) / dt / 1e9) for (a, b, dt, up) in rows]
    if not quiet:
        print(f"B={B} resident: {1e3 * dt_res:8.2f} ms/batch-iteration = {B / dt_res:9.1f} trajectory-iterations/s")
        for r in out["rows"]:
            print(f"B={B} {r['payload']:36s} {r['form']:32s}: {r['ms_per_iteration']:8.2f} ms = {r['traj_it_per_s']:9.1f} traj-it/s"
                  f"  (H2D {r['h2d_GB']:.2f} GB + D2H {r['d2h_GB']:.2f} GB -> {r['link_GBps']:.1f} GB/s)", flush=True)
    return out


def measure_gains(B=256, steps=10, rounds=3, T=3000, nchunks=3, quiet=False):
    uniq = min(8, B)
    p = synth.tile_problem(synth.make_problem(task="panda_reaching", T=T, batch=uniq, min_N=5), B // uniq)
    B = p["batch"]
    with Engine(p["dof"], p["m"], T, p["nr"], batch=B, fused=True) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=True)
        e.iterate(p["lam"], 100, np.array([(i / 6.0) ** 2 for i in range(1, 7)])); e.sync()
        K0, k0 = e.gains()
        r = e.pinned(p["r"].shape); r[...] = p["r"]
        lam = e.pinned(B); lam[:] = p["lam"]
        slab = e.fd_kp_slab(*synth.kp_ordered_payload(p))
        half = np.sort(np.random.default_rng(5).permutation(B)[:B // 2]).astype(np.int32)      # scattered: runs of every length
        H = len(half)
        K = e.pinned(K0.shape); k = e.pinned(k0.shape); K32 = e.pinned(K0.shape, np.float32)
        Kh = e.pinned((H,) + K0.shape[1:]); kh = e.pinned((H,) + k0.shape[1:]); K32h = e.pinned((H,) + K0.shape[1:], np.float32)
        legs = [("1 FP64 K, kpilqr_iterate_streamed", dict(K=K, k=k), K.nbytes + k.nbytes)]
        if hasattr(e._L, "kpilqr_iterate_streamed2"):
            legs += [("2 K32, whole batch", dict(K32=K32, k=k), K32.nbytes + k.nbytes),
                     ("3 K32, scattered half listed", dict(K32=K32h, k=kh, gain_traj=half), K32h.nbytes + kh.nbytes),
                     ("4 FP64 K, the same half listed", dict(K=Kh, k=kh, gain_traj=half), Kh.nbytes + kh.nbytes)]
        up = slab["layout"].bytes + r.nbytes

        def run(kw):
            e.iterate_streamed(fd_kp=slab, eps=p["eps"], r=r, lam=lam, nchunks=nchunks, **kw)

        for _, kw, _ in legs:
            run(kw); run(kw)
        e.sync()
        # (the :rxc sweeps: K in the bits of the staged path, k to 1e-12 -- as in measure())
        assert np.array_equal(K, K0) and np.max(np.abs(k - k0)) <= 1e-12 * np.max(np.abs(k0))
        if len(legs) > 1:
            with np.errstate(under="ignore"):
                assert np.array_equal(K32, K0.astype(np.float32)) and np.array_equal(K32h, K0[half].astype(np.float32))
            assert np.array_equal(Kh, K0[half]) and np.array_equal(kh, k[half])
        times = [[] for _ in legs]
        for _ in range(rounds):
            for i, (_, kw, _) in enumerate(legs):
                t0 = time.perf_counter()
                for _ in range(steps):
                    run(kw)
                e.sync()
                times[i].append((time.perf_counter() - t0) / steps)
    rows = []
    for (label, _, dn), ts in zip(legs, times):
        dt = float(np.median(ts))
        rows.append(dict(leg=label, ms_per_iteration=1e3 * dt, ms_rounds=[round(1e3 * t, 3) for t in ts], traj_it_per_s=B / dt,
                         h2d_GB=up / 1e9, d2h_GB=dn / 1e9, link_GBps=(up + dn) / dt / 1e9, rate_vs_leg1=float(np.median(times[0])) / dt))
    if not quiet:
        for r_ in rows:
            print(f"B={B} {r_['leg']:34s}: {r_['ms_per_iteration']:8.2f} ms (rounds {r_['ms_rounds']}) = {r_['traj_it_per_s']:9.1f} traj-it/s  x{r_['rate_vs_leg1']:.3f}"
                  f"  (H2D {r_['h2d_GB']:.3f} GB + D2H {r_['d2h_GB']:.3f} GB -> {r_['link_GBps']:.1f} GB/s)", flush=True)
    return dict(batch=B, T=T, steps=steps, rounds=rounds, nchunks=nchunks, rows=rows)


def measure_columns(B=256, steps=10, rounds=3, T=3000, nchunks=3, quiet=False):
    uniq = min(8, B)
    p = synth.tile_problem(synth.make_problem(task="panda_reaching", T=T, batch=uniq, min_N=5), B // uniq)
    B = p["batch"]
    with Engine(p["dof"], p["m"], T, p["nr"], batch=B, fused=True) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=True)
        alphas = np.array([(i / 6.0) ** 2 for i in range(1, 7)])
        r = e.pinned(p["r"].shape); r[...] = p["r"]
        u_nom = e.pinned(p["u_nom"].shape); u_nom[...] = p["u_nom"]
        lam = e.pinned(B); lam[:] = p["lam"]
        payload = synth.kp_ordered_payload(p)
        slab = e.fd_kp_slab(*payload)
        cols = e.kp_columns(*payload, eps=p["eps"])
        E, n = cols["entries"], p["n"]
        dofs = synth.kp_entry_dofs(p)
        c32 = e.pinned(E * 3 * n, np.float32)
        c32[...] = synth.encode_kp_columns_f32(cols["cols"][:E * 3 * n].reshape(E, 3, n), dofs, p["dof"]).reshape(-1)
        # the yardsticks of the two payloads: the staged path on the FP64 columns, and on the numpy-decoded FP32 ones
        e.upload_kp_columns(cols); e.iterate(p["lam"], 100, alphas); e.sync()
        K0, k0 = e.gains()
        dec = dict(cols=np.ascontiguousarray(synth.decode_kp_columns_f32(np.asarray(c32).reshape(E, 3, n), dofs, p["dof"]).reshape(-1)), entries=E)
        e.upload_kp_columns(dec); e.iterate(p["lam"], 100, alphas); e.sync()
        K1, k1 = e.gains()
        K = e.pinned(K0.shape); k = e.pinned(k0.shape); K32 = e.pinned(K0.shape, np.float32)
        same_up = r.nbytes + u_nom.nbytes + lam.nbytes
        col64, col32 = E * 3 * n * 8, E * 3 * n * 4
        legs = [("0 x+ / x- key-point ordered, FP64 K", e.iterate_streamed, dict(fd_kp=slab, K=K, k=k), slab["layout"].bytes, K.nbytes + k.nbytes),
                ("1 FP64 columns, kpilqr_iterate_streamed", e.iterate_streamed, dict(kp_cols=cols, K=K, k=k), col64, K.nbytes + k.nbytes)]
        if hasattr(e._L, "kpilqr_iterate_streamed3"):
            legs += [("2 FP32 columns, kpilqr_iterate_streamed3", e.iterate_streamed3, dict(kp_cols32=c32, K=K, k=k), col32, K.nbytes + k.nbytes),
                     ("3 FP32 columns and K32", e.iterate_streamed3, dict(kp_cols32=c32, K32=K32, k=k), col32, K32.nbytes + k.nbytes)]

        def run(fn, kw):
            fn(eps=p["eps"], r=r, u_nom=u_nom, lam=lam, nchunks=nchunks, **kw)

        def close(k_got, k_want):      # (the :rxc sweeps: K in the bits of the staged path, k to 1e-12 -- as in measure())
            return np.max(np.abs(k_got - k_want)) <= 1e-12 * np.max(np.abs(k_want))

        for label, fn, kw, _, _ in legs:
            K[...] = 0; K32[...] = 0
            run(fn, kw); run(fn, kw)
            e.sync()
            if label[0] in "01":
                assert np.array_equal(K, K0) and close(k, k0), label
            elif label[0] == "2":
                assert np.array_equal(K, K1) and close(k, k1), label
            else:
                with np.errstate(under="ignore"):
                    assert np.array_equal(K32, K1.astype(np.float32)) and close(k, k1), label
        times = [[] for _ in legs]
        for _ in range(rounds):
            for i, (_, fn, kw, _, _) in enumerate(legs):
                t0 = time.perf_counter()
                for _ in range(steps):
                    run(fn, kw)
                e.sync()
                times[i].append((time.perf_counter() - t0) / steps)
        moved = float(np.max(np.abs(K1 - K0)) / np.max(np.abs(K0)))
    rows = []
    for (label, _, _, up, dn), ts in zip(legs, times):
        dt = float(np.median(ts))
        rows.append(dict(leg=label, ms_per_iteration=1e3 * dt, ms_rounds=[round(1e3 * t, 3) for t in ts], traj_it_per_s=B / dt,
                         h2d_MB_per_traj=(up + same_up) / B / 1e6, d2h_MB_per_traj=dn / B / 1e6, link_GBps=(up + same_up + dn) / dt / 1e9,
                         rate_vs_leg1=float(np.median(times[1])) / dt))
    if not quiet:
        for r_ in rows:
            print(f"B={B} {r_['leg']:42s}: {r_['ms_per_iteration']:8.2f} ms (rounds {r_['ms_rounds']}) = {r_['traj_it_per_s']:9.1f} traj-it/s  x{r_['rate_vs_leg1']:.3f}"
                  f"  (H2D {r_['h2d_MB_per_traj']:.3f} MB + D2H {r_['d2h_MB_per_traj']:.3f} MB per trajectory -> {r_['link_GBps']:.1f} GB/s)", flush=True)
        print(f"B={B} the FP32 transport moves K by {moved:.2e} relative (max |dK| / max |K|, staged path on both payloads)", flush=True)
    return dict(batch=B, T=T, steps=steps, rounds=rounds, nchunks=nchunks, rows=rows, K_moved_by_f32_columns=moved)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "columns":
        a = [int(x) for x in sys.argv[2:]]
        measure_columns(*a)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "gains":
        a = [int(x) for x in sys.argv[2:]]
        measure_gains(*a)
        sys.exit(0)
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    chunks = tuple(int(x) for x in sys.argv[3].split(",")) if len(sys.argv) > 3 else (4, 8, 16)
    measure(B, steps, chunk_list=chunks)
