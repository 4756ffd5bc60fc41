"""Inputs for which the control clamp of the forward sweeps (iLQR.cpp:883-889: U = clamp(u_nom + K dx + alpha k, lo, hi), du = U -
u_nom) is really active, chosen with the CPU oracle alone.  The problems of synth.make_problem / make_ragged_problem keep every
control well inside its limits; activate() replaces u_nom and ctrl_lim -- which the backward sweep never reads, so gains and
derivatives stay what they were -- such that about 30 % of the controls of every alpha sit on a limit, on both limits of every
control, and on a different set of entries from one alpha to the next.  tests/test_clamp_cases.py holds every case of
tests/_shapes.py to the conditions below without a GPU; tests/test_gpu_clamp.py runs them on the device."""
import numpy as np

from oracle import oracle as orc
from oracle import pipeline

WIDE = 1e30                         # a limit no control reaches
SHARE = (0.15, 0.45)                # the conditions a clamp case meets on the oracle: share of U_alpha entries exactly on a limit,
MIN_HITS = 2                        # hits of every control on each of its two limits,
MIN_DIFFER = 3                      # entries whose on-limit flag differs between the first and the last alpha (n_alpha > 1)


def linearise(p):
    """The oracle up to the gains, one dict per trajectory: what every forward run of a problem shares, whatever its u_nom and
    limits."""
    return [pipeline.run_trajectory(p, b, stages=("fd", "interp", "cost", "bwd")) for b in range(p["batch"])]


def forward(p, lin, n_alpha, u_nom=None, ctrl_lim=None):
    """orc.forward_linear on the gains of lin: [(cost_pred, U_alpha) or None where the backward status is non-zero]."""
    u_nom = p["u_nom"] if u_nom is None else u_nom
    ctrl_lim = p["ctrl_lim"] if ctrl_lim is None else ctrl_lim
    al = orc.alphas(n_alpha)
    return [orc.forward_linear(p["n"], p["m"], p["T"], al, o["A"], o["B"], o["K"], o["k"], o["l_x"], o["l_xx"], o["l_u"], o["l_uu"],
                               u_nom[b], ctrl_lim, want_U=True) if o["status"] == 0 else None
            for b, o in enumerate(lin)]


def references(p, n_alpha, lin=None):
    """What pipeline.run_trajectory(p, b, n_alpha=n_alpha, want_U=True) returns for every trajectory, the backward pass taken from lin."""
    lin = linearise(p) if lin is None else lin
    return [dict(o) if r is None else dict(o, cost_pred=r[0], U_alpha=r[1], alphas=orc.alphas(n_alpha))
            for o, r in zip(lin, forward(p, lin, n_alpha))]


def _pooled(runs, m):
    """U_alpha of the trajectories that ran, pooled over batch, alphas and steps: [samples, m]."""
    return np.concatenate([r[1].reshape(-1, m) for r in runs if r is not None])


def _wide(m):
    return np.tile([-WIDE, WIDE], m)


def unclamped(p, n_alpha, lin=None):
    """The pooled controls [samples, m] of p's u_nom with no limit."""
    lin = linearise(p) if lin is None else lin
    return _pooled(forward(p, lin, n_alpha, ctrl_lim=_wide(p["m"])), p["m"])


def activate(p, n_alpha, lin=None, q=(0.15, 0.85)):
    """A copy of p with u_nom rescaled per control to the RMS of the feedback term alpha k + K dx, and with limits midway between
    the order statistics of the unclamped controls at the quantiles q (so that no unclamped sample sits on a limit): asymmetric,
    different for every control, and cutting into u_nom itself."""
    lin = linearise(p) if lin is None else lin
    m = p["m"]
    ok = [b for b, o in enumerate(lin) if o["status"] == 0]
    assert ok, "no trajectory of the problem has a positive-definite backward pass"
    fb = _pooled(forward(p, lin, n_alpha, u_nom=np.zeros_like(p["u_nom"]), ctrl_lim=_wide(m)), m)
    rms_fb = np.sqrt(np.mean(fb ** 2, axis=0))
    rms_u = np.sqrt(np.mean(p["u_nom"][ok].reshape(-1, m) ** 2, axis=0))
    assert np.all(rms_fb > 0) and np.all(rms_u > 0), (rms_fb, rms_u)
    q_ = dict(p)
    q_["u_nom"] = p["u_nom"] * (rms_fb / rms_u)[None, None, :]
    s = np.sort(_pooled(forward(q_, lin, n_alpha, ctrl_lim=_wide(m)), m), axis=0)
    N = s.shape[0]
    i, j = int(np.floor(q[0] * N)), int(np.ceil(q[1] * N))
    assert 1 <= i < j <= N - 1, (N, i, j)
    lo, hi = 0.5 * (s[i - 1] + s[i]), 0.5 * (s[j - 1] + s[j])
    q_["ctrl_lim"] = np.stack([lo, hi], axis=1).reshape(-1)
    return q_


def on_limit(U, ctrl_lim):
    """Boolean mask of the entries of U [..., m] exactly on a limit."""
    return (U == ctrl_lim[0::2]) | (U == ctrl_lim[1::2])


def conditions(p, n_alpha, lin=None):
    """From the oracle's run of p as it stands: the share of U_alpha entries exactly on a limit, the minimum over controls of the
    hits on lo and on hi, the number of entries whose on-limit flag differs between the first and the last alpha, and the number
    of trajectories that ran."""
    lin = linearise(p) if lin is None else lin
    runs = [r for r in forward(p, lin, n_alpha) if r is not None]
    U = np.stack([r[1] for r in runs])                                      # [ran, n_alpha, T, m]
    lo, hi = p["ctrl_lim"][0::2], p["ctrl_lim"][1::2]
    on = on_limit(U, p["ctrl_lim"])
    return dict(share=float(on.mean()), hits_lo=int((U == lo).sum(axis=(0, 1, 2)).min()), hits_hi=int((U == hi).sum(axis=(0, 1, 2)).min()),
                differ=int((on[:, 0] != on[:, -1]).sum()), ran=len(runs), clamped=int(on.sum()),
                cost=np.stack([r[0] for r in runs]))


def assert_conditions(cond, n_alpha, tag=""):
    assert SHARE[0] <= cond["share"] <= SHARE[1], (tag, cond)
    assert cond["hits_lo"] >= MIN_HITS and cond["hits_hi"] >= MIN_HITS, (tag, cond)
    assert n_alpha == 1 or cond["differ"] >= MIN_DIFFER, (tag, cond)


def edge_limits(p, n_alpha, lin=None):
    """A copy of an activated problem with control 0 pinned (lo = hi = its pooled median), the last control unlimited at +-1e300 (the
    kernels' own pad sentinel) and control m - 2 (m >= 3) limited from above only."""
    m = p["m"]
    lim = p["ctrl_lim"].copy()
    lim[0] = lim[1] = float(np.median(unclamped(p, n_alpha, lin)[:, 0]))
    if m >= 3:
        lim[2 * (m - 2)] = -1e300
    lim[2 * (m - 1)], lim[2 * (m - 1) + 1] = -1e300, 1e300          # (m = 1: the one control is the unlimited one)
    return dict(p, ctrl_lim=lim)
