"""Timing of iLQR_SVR's singular-vector DoF importance on the device (kpilqr_dof_importance_svd, hipEvents on the context's
stream) next to the path it replaces: kpilqr_download_gains of all of K (hipEvents, pageable destination as a caller's
array) plus host/SVR.cpp's ThinSVD-based DofImportance over the trajectories on 16 host threads.

    python tools/svr_timing.py [--out FILE]

Gains are random (16 distinct trajectories tiled over the batch, state-column scales spread by exp(U(-3, 2))) and injected
into KPILQR_BUF_K; the device sums are checked against the host's on 16 trajectories."""
import argparse
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajoptkp_amd import Engine, host  # noqa: E402

CASES = [("panda", 7, 7, 1024, 3000, 1), ("panda", 7, 7, 1024, 3000, 10), ("n=62", 31, 7, 128, 5000, 1)]
HOST_THREADS = 16


def event_ms(stream, fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(); b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def run(name, dof, m, B, T, s, lines):
    rng = np.random.default_rng(dof * 1000 + s)
    n = 2 * dof
    K16 = rng.standard_normal((16, T, n, m)) * np.exp(rng.uniform(-3, 2, (16, 1, n, 1)))
    K = np.ascontiguousarray(np.tile(K16, (B // 16, 1, 1, 1)))
    stream = torch.cuda.Stream()
    with Engine(dof, m, T, 2, batch=B, stream=stream.cuda_stream) as e:
        with torch.cuda.stream(stream):
            torch.as_tensor(e.device_array(1, K.shape), device="cuda").copy_(torch.from_numpy(K))
        stream.synchronize()
        L, h = e._L, e._h
        sums = np.zeros((B, dof))
        Kd = np.empty_like(K)
        svd = lambda: e._ck(L.kpilqr_dof_importance_svd(h, s, sums.ctypes.data_as(C.c_void_p)))
        dl = lambda: e._ck(L.kpilqr_download_gains(h, Kd.ctypes.data_as(C.c_void_p), None))
        svd(); e.sync()                                            # staging allocated, code objects loaded
        dev_med, dev_min = event_ms(stream, svd, 5)
        dl(); e.sync()
        dl_med, dl_min = event_ms(stream, dl, 3)
        e.sync()
    assert np.array_equal(Kd, K)
    worst = 0.0
    for b in range(16):
        ref = host.dof_importance(K16[b], dof, s, svd=True)[0]
        worst = max(worst, float(np.max(np.abs(sums[b] - ref)) / np.max(ref)))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        list(ex.map(lambda b: host.dof_importance(Kd[b], dof, s, svd=True), range(B)))
    host_ms = (time.perf_counter() - t0) * 1e3
    ns = (T + s - 1) // s
    line = (f"{name:6s} n={n:2d} m={m} B={B:4d} T={T} s={s:2d}: {B * ns / 1e6:5.2f} M SVDs | device {dev_med:8.2f} ms "
            f"(min {dev_min:.2f}) | download K {K.nbytes / 1e9:.2f} GB {dl_med:7.2f} ms (min {dl_min:.2f}) + host ThinSVD on "
            f"{HOST_THREADS} threads {host_ms:8.1f} ms | device / download {dev_med / dl_med:.2f} | max rel diff to host (16 traj.) {worst:.1e}")
    print(line, flush=True)
    lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}; times: median of 5 (device) / 3 (download) event-timed calls"]
    for c in CASES:
        run(*c, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
