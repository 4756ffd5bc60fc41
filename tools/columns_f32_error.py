"""What rounding the key-point columns to FP32 does to the results, on the CPU (no GPU, no library): the numpy restatement of
oracle/crosscheck.py -- np_fd -> round the key-point columns -> np_interp -> np_backward / np_forward -- against the same run on the
unrounded FP64 columns, for the two encodings a caller could choose:

    plain    (float) of every column element
    unit     the encoding of kpilqr_upload_kp_columns_f32 (include/kpilqr.h): A's unit entry removed, in double, before the cast,
             and added back after the widening

    python tools/columns_f32_error.py [--quick] [--out FILE]

Workloads are the synthetic ones of trajoptkp_amd.synth.make_problem (stand-in dynamics, not MuJoCo).  Error = max-norm relative
change, max |x - x_ref| / max |x_ref|, against the unrounded run; "(float)K" is what the FP32 gain download costs on the same gains,
for scale.  --quick: T cut to a tenth (a smoke run of the tool itself; the committed table is the full run)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import crosscheck as cc  # noqa: E402
from trajoptkp_amd import synth  # noqa: E402

LAMS = (1e-4, 0.1, 10.0)
# name, make_problem arguments, lambdas
CASES = [
    ("panda_reaching T=3000", dict(task="panda_reaching", T=3000, batch=1, min_N=5, config_id=2), LAMS),
    ("panda_reaching dense r_x T=600", dict(task="panda_reaching", T=600, batch=1, min_N=5, config_id=2, dense_residuals=True), (0.1, 10.0)),
    ("acrobot T=600", dict(task="acrobot", T=600, batch=1, min_N=5, config_id=1), LAMS),
    ("panda_pushing T=300", dict(task="panda_pushing", T=300, batch=1, min_N=4, config_id=3), LAMS),
]


def round_keypoint_columns(p, b, A, B, encoding):
    """A, B of np_fd (maths layout M[t, row, col], non-zero at the key-points) with every key-point column through FP32 and back.
    encoding: "plain" | "unit".  Returns the rounded copies and the number of elements of A that changed."""
    dof, m, T = p["dof"], p["m"], p["T"]
    offs, cols = p["kp_rows"][b]
    t_of = np.repeat(np.arange(T), np.diff(offs))
    A2 = A.copy(); B2 = B.copy()
    for i in range(dof):
        ts = np.unique(t_of[cols == i])
        for c in (i, i + dof):
            col = A[ts, :, c].copy()
            if encoding == "unit":
                col[:, c] -= 1.0
            col = col.astype(np.float32).astype(np.float64)
            if encoding == "unit":
                col[:, c] += 1.0
            A2[ts, :, c] = col
        if i < m:
            B2[ts, :, i] = B[ts, :, i].astype(np.float32).astype(np.float64)
    return A2, B2, int(np.count_nonzero(A2 != A))


def run(p, b, A, B, lam, n_alpha=6):
    A, B = cc.np_interp(p, b, A, B)
    l_x, l_xx, l_u, l_uu = cc.np_cost(p, b)
    st, K, k, dJ = cc.np_backward(A, B, l_x, l_xx, l_u, l_uu, lam)
    alphas = (np.arange(1, n_alpha + 1) / n_alpha) ** 2
    cost, U = cc.np_forward(A, B, K, k, l_x, l_xx, l_u, l_uu, p["u_nom"][b], p["ctrl_lim"], alphas)
    return dict(status=st, K=K, k=k, delta_J=np.array(dJ), cost_pred=cost, U_alpha=U)


def errors(p, b, lam):
    """{encoding: {K, k, delta_J, cost_pred, U_alpha: relative change, changed: elements of A}} and the (float)K scale"""
    A, B = cc.np_fd(p, b)
    ref = run(p, b, A, B, lam)
    assert ref["status"] == 0
    out = {}
    for enc in ("plain", "unit"):
        A2, B2, changed = round_keypoint_columns(p, b, A, B, enc)
        got = run(p, b, A2, B2, lam)
        assert got["status"] == 0
        out[enc] = {key: cc.rel(got[key], ref[key]) for key in ("K", "k", "delta_J", "cost_pred", "U_alpha")}
        out[enc]["changed"] = changed
    return out, cc.rel(ref["K"].astype(np.float32).astype(np.float64), ref["K"])


def byte_model():
    """Bytes per trajectory on the headline shape: Panda reaching, T = 3000, key-points every 5 steps"""
    dof, m, T, min_N = 7, 7, 3000, 5
    n = 2 * dof
    offs, _ = synth.keypoint_rows_set_interval(dof, T, min_N)
    entries = dof * int(np.count_nonzero(np.diff(offs)))
    return [f"  key-point entries per trajectory: {entries}",
            f"  x+ / x- payload (kpilqr_upload_fd_kp, (6n + 2) * 8 bytes per entry)   {entries * (6 * n + 2) * 8 / 1e6:5.2f} MB",
            f"  FP64 key-point columns (kpilqr_upload_kp_columns, 3n * 8)             {entries * 3 * n * 8 / 1e6:5.2f} MB",
            f"  FP32 key-point columns (kpilqr_upload_kp_columns_f32, 3n * 4)         {entries * 3 * n * 4 / 1e6:5.2f} MB",
            f"  K down as FP32 (T*n*m*4) plus k (T*m*8)                               {(T * n * m * 4 + T * m * 8) / 1e6:5.2f} MB"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["case, lambda | plain (float): K k delta_J cost_pred U_alpha | unit entry removed: K k delta_J cost_pred U_alpha | (float)K | elements of A changed (plain / unit)"]
    worst = {}
    for name, kw, lams in CASES:
        if a.quick:
            kw = dict(kw, T=max(kw["T"] // 10, 30))
            name += f" (quick: T={kw['T']})"
        p = synth.make_problem(**kw)
        for lam in lams:
            e, scale = errors(p, 0, lam)
            fmt = lambda d: " ".join(f"{d[key]:.1e}" for key in ("K", "k", "delta_J", "cost_pred", "U_alpha"))
            line = f"{name:32s} lambda={lam:<6g} | {fmt(e['plain'])} | {fmt(e['unit'])} | {scale:.1e} | {e['plain']['changed']} / {e['unit']['changed']}"
            print(line, flush=True)
            lines.append(line)
            for enc in e:
                for key, v in e[enc].items():
                    if key != "changed":
                        worst[(enc, key)] = max(worst.get((enc, key), 0.0), v)
    lines.append("worst over the cases: " + "; ".join(f"{enc}: " + ", ".join(f"{key} {worst[(enc, key)]:.1e}" for key in ("K", "k", "delta_J", "cost_pred", "U_alpha"))
                                                        for enc in ("plain", "unit")))
    print(lines[-1])
    lines += ["", "Byte model (per trajectory, Panda reaching, T = 3000, key-points every 5 steps)"] + byte_model()
    print("\n".join(lines[-6:]))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
