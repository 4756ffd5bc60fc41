"""What symmetrising Qzz IN FRONT of the gains instead of V' behind them does to the backward sweep, on the CPU (no GPU, no library):
a numpy restatement of the recursion of the one-wave sweeps (fused_mfma.hip, `step`) in the augmented state z = [x; 1] on the oracle's
A, B, l_* (oracle/pipeline.py), run in two variants that share every statement but the last:

    (a)  V = sym(Qzz + K'G)        as the sweeps did it: the transposition behind the last product of the step
    (b)  V = sym(Qzz) + K'G        the transposition in front of the refresh; V keeps the rounding asymmetry of ONE product K'G

with Qr = Luu + lambda I + Fu'V'Fu, Quz = Luz + Fu'V'Fz, Qzz = Lzz + Fz'V'Fz, K = -Qr^-1 Quz (gains with their sign, k in column n),
G = Quz - lambda K, element (n, n) of V zeroed, delta_J = -lambda sum k'k.  K'G is the same plain (un-symmetrised) product in both.

    python tools/early_symmetrise_error.py [--quick] [--out FILE]

Workloads are the synthetic ones of trajoptkp_amd.synth.make_problem (stand-in dynamics, not MuJoCo).  Reported per workload and
lambda, worst over the seeds: max-norm relative difference of K, k and delta_J between (a) and (b), and the worst
max|V - V'| / max|V| along the sweep of (b).  GATE: the difference of K stays below 1e-13, a decade under the 1e-12 at which the tests
hold kernel forms to one another.  --quick: T = 64, two seeds (tests/test_early_symmetrise_model.py runs that)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pipeline  # noqa: E402
from trajoptkp_amd import synth  # noqa: E402

GATE = 1e-13
LAMS = (1e-4, 1e-2, 0.1, 1.0, 10.0)
# name, make_problem arguments (batch = seeds: seed_for(config_id, 0 .. batch-1), the family of the headline's distinct seeds)
CASES = [
    ("panda_reaching T=3000", dict(task="panda_reaching", T=3000, batch=8, min_N=5, config_id=2)),
    ("acrobot T=1000", dict(task="acrobot", T=1000, batch=2, min_N=5, config_id=1)),
    ("panda_reaching r_u != 0 T=600", dict(task="panda_reaching", T=600, batch=2, min_N=5, config_id=2, dense_residuals=True)),
]


def tiles(p, b):
    """The oracle's A, B, l_* of trajectory b as the per-step tiles of the augmented recursion (maths layout M[t, row, col])"""
    o = pipeline.run_trajectory(p, b, stages=("fd", "interp", "cost"))
    T, n, m = p["T"], p["n"], p["m"]
    Fz = np.zeros((T, n + 1, n + 1)); Fu = np.zeros((T, n + 1, m))
    Fz[:, :n, :n] = np.swapaxes(o["A"], 1, 2); Fz[:, n, n] = 1.0
    Fu[:, :n, :] = np.swapaxes(o["B"], 1, 2)
    Lzz = np.zeros((T, n + 1, n + 1)); Luz = np.zeros((T, m, n + 1))
    Lzz[:, :n, :n] = np.swapaxes(o["l_xx"], 1, 2); Lzz[:, :n, n] = o["l_x"]; Lzz[:, n, :n] = o["l_x"]
    Luz[:, :, n] = o["l_u"]
    return Fz, Fu, Lzz, Luz, np.swapaxes(o["l_uu"], 1, 2)


def sweep(Fz, Fu, Lzz, Luz, Luu, lam, early):
    """-> K [T, m, n], k [T, m], delta_J, worst asymmetry of V.  early: variant (b)"""
    T, n1, m = Fu.shape
    n = n1 - 1
    K = np.zeros((T, m, n)); k = np.zeros((T, m))
    V = Lzz[T - 1].copy(); V[n, n] = 0.0
    dJ, asym = 0.0, 0.0
    I = np.eye(m)
    for t in range(T - 1, -1, -1):
        Tu = V.T @ Fu[t]; Tz = V.T @ Fz[t]
        Qr = Luu[t] + lam * I + Fu[t].T @ Tu
        Quz = Luz[t] + Fu[t].T @ Tz
        Qzz = Lzz[t] + Fz[t].T @ Tz
        Kp = -np.linalg.solve(Qr, Quz)
        K[t] = Kp[:, :n]; k[t] = Kp[:, n]
        dJ += k[t] @ k[t]
        KG = Kp.T @ (Quz - lam * Kp)
        if early:
            V = 0.5 * (Qzz + Qzz.T) + KG
        else:
            Vp = Qzz + KG
            V = 0.5 * (Vp + Vp.T)
        V[n, n] = 0.0
        asym = max(asym, float(np.max(np.abs(V - V.T)) / np.max(np.abs(V))))
    return K, k, -lam * dJ, asym


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


def study(kw, lams=LAMS):
    """{lambda: dict(K, k, delta_J, asym)}: worst over the seeds of the problem"""
    p = synth.make_problem(**kw)
    out = {lam: dict(K=0.0, k=0.0, delta_J=0.0, asym=0.0) for lam in lams}
    for b in range(p["batch"]):
        tl = tiles(p, b)
        for lam in lams:
            Ka, ka, dJa, _ = sweep(*tl, lam, early=False)
            Kb, kb, dJb, asym = sweep(*tl, lam, early=True)
            w = out[lam]
            w["K"] = max(w["K"], rel(Kb, Ka)); w["k"] = max(w["k"], rel(kb, ka))
            w["delta_J"] = max(w["delta_J"], abs(dJb - dJa) / abs(dJa)); w["asym"] = max(w["asym"], asym)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["case (seeds), lambda | (b) against (a): K k delta_J | worst |V - V'| / |V| in (b)"]
    worst_K, over = 0.0, []
    for name, kw in CASES:
        if a.quick:
            kw = dict(kw, T=64, batch=2)
            name += " (quick: T=64)"
        for lam, w in study(kw).items():
            line = f"{name:34s} ({kw['batch']}) lambda={lam:<6g} | {w['K']:.1e} {w['k']:.1e} {w['delta_J']:.1e} | {w['asym']:.1e}"
            print(line, flush=True)
            lines.append(line)
            worst_K = max(worst_K, w["K"])
            if not w["K"] < GATE:
                over.append(f"{name} lambda={lam:g}")
    lines.append(f"worst relative difference of K: {worst_K:.1e}   gate {GATE:.0e}: " + ("holds" if not over else "EXCEEDED by " + "; ".join(over)))
    print(lines[-1])
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    return 1 if over else 0


if __name__ == "__main__":
    sys.exit(main())
