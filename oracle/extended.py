"""The backward and forward sweeps in extended precision (numpy longdouble, a 64-bit mantissa on x86): a third implementation
beside the C oracle and oracle/crosscheck.py's numpy restatement, whose arithmetic it repeats (np_backward / np_forward), to
measure what float64 rounding does to either of them -- and to a GPU sweep -- on a given problem.

TEST INFRASTRUCTURE ONLY (see oracle/kpilqr_oracle.h).  tests/_blockwise.py takes its bars from it; tools/wide_error_budget.py
its error budget."""
import numpy as np

from . import crosscheck as cc
from . import oracle as orc
from . import pipeline

LD = np.longdouble


def ld_solve(M, R):
    """M^-1 R, Gaussian elimination with partial pivoting in longdouble."""
    M = M.astype(LD).copy(); R = R.astype(LD).copy()
    m = M.shape[0]
    for j in range(m):
        p = j + int(np.argmax(np.abs(M[j:, j])))
        if p != j:
            M[[j, p]] = M[[p, j]]; R[[j, p]] = R[[p, j]]
        piv = M[j, j]
        f = M[j + 1:, j] / piv
        M[j + 1:] -= f[:, None] * M[j][None, :]
        R[j + 1:] -= f[:, None] * R[j][None, :]
    for j in range(m - 1, -1, -1):
        R[j] = (R[j] - M[j, j + 1:] @ R[j + 1:]) / M[j, j]
    return R


def ld_backward(A, B, l_x, l_xx, l_u, l_uu, lam):
    A, B, l_x, l_xx, l_u, l_uu = (x.astype(LD) for x in (A, B, l_x, l_xx, l_u, l_uu))
    T, n, m = A.shape[0], A.shape[1], B.shape[2]
    K = np.zeros((T, m, n), LD); k = np.zeros((T, m), LD)
    Vx = l_x[T - 1].copy(); Vxx = l_xx[T - 1].copy()
    dJ = LD(0)
    I = np.eye(m, dtype=LD)
    for t in range(T - 1, -1, -1):
        Qx = l_x[t] + A[t].T @ Vx
        Qu = l_u[t] + B[t].T @ Vx
        Qxx = l_xx[t] + A[t].T @ Vxx @ A[t]
        Quu = l_uu[t] + B[t].T @ Vxx @ B[t]
        Qux = B[t].T @ Vxx @ A[t]
        inv = ld_solve(Quu + LD(lam) * I, I)
        k[t] = -inv @ Qu
        K[t] = -inv @ Qux
        Vx = Qx + K[t].T @ (Quu @ k[t]) + K[t].T @ Qu + Qux.T @ k[t]
        Vxx = Qxx + K[t].T @ (Quu @ K[t]) + K[t].T @ Qux + Qux.T @ K[t]
        Vxx = (Vxx + Vxx.T) / 2
        dJ += k[t] @ Qu + k[t] @ Quu @ k[t]
    return K, k, dJ


def ld_forward(A, B, K, k, l_x, l_xx, l_u, l_uu, u_nom, ctrl_lim, alphas):
    A, B, K, k, l_x, l_xx, l_u, l_uu, u_nom = (np.asarray(x).astype(LD) for x in (A, B, K, k, l_x, l_xx, l_u, l_uu, u_nom))
    T, n, m = A.shape[0], A.shape[1], B.shape[2]
    lo, hi = ctrl_lim[0::2].astype(LD), ctrl_lim[1::2].astype(LD)
    cost = np.zeros(len(alphas), LD); U = np.zeros((len(alphas), T, m), LD)
    for a, alpha in enumerate(alphas):
        dx = np.zeros(n, LD)
        for t in range(T):
            u = np.clip(u_nom[t] + LD(alpha) * k[t] + K[t] @ dx, lo, hi)
            du = u - u_nom[t]
            U[a, t] = u
            cost[a] += l_x[t] @ dx + LD(0.5) * (dx @ l_xx[t] @ dx) + l_u[t] @ du + LD(0.5) * (du @ l_uu[t] @ du)
            dx = A[t] @ dx + B[t] @ du
    return cost, U


def extended_trajectory(p, b, lam=None, n_alpha=6, pd_stride=100):
    """Trajectory b of problem p through ld_backward / ld_forward on the A, B, l_* of pipeline.run_trajectory (the stages before
    the sweeps are bit-exact on the GPU and are not what this measures).  Returns longdouble K [T][n][m], k, delta_J, cost_pred
    and U_alpha in the oracle's column-major-per-step layout, with status 0; where the oracle's PD check fails, its status and
    nothing else."""
    lam = p["lam"] if lam is None else lam
    o = pipeline.run_trajectory(p, b, lam=lam, pd_stride=pd_stride, n_alpha=n_alpha, stages=("fd", "interp", "cost", "bwd"))
    if o["status"] != 0:
        return dict(status=o["status"])
    A, B = cc._T(o["A"]), cc._T(o["B"])
    l_x, l_xx, l_u, l_uu = o["l_x"], cc._T(o["l_xx"]), o["l_u"], cc._T(o["l_uu"])
    K, k, dJ = ld_backward(A, B, l_x, l_xx, l_u, l_uu, lam)
    cost, U = ld_forward(A, B, K, k, l_x, l_xx, l_u, l_uu, p["u_nom"][b], p["ctrl_lim"], orc.alphas(n_alpha))
    return dict(status=0, K=np.ascontiguousarray(cc._T(K)), k=k, delta_J=dJ, cost_pred=cost, U_alpha=U)
