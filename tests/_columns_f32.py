"""Shared by tests/test_columns_f32_abi.py (CPU) and tests/test_gpu_columns_f32.py: key-point columns [entries][3][n] of a synthetic
problem put back where the restatements of the pipeline expect them, so that the numpy restatement (oracle/crosscheck.py) and the C
oracle can be run ON the columns the FP32 transport delivers."""
import numpy as np

from oracle import oracle as orc
from trajoptkp_amd.engine import rows_to_dof_csr


def entry_csr(p):
    """(offsets [batch*dof + 1], times [entries]) of a problem's per-DoF key-point lists: the CSR the columns are ordered by"""
    return rows_to_dof_csr(p["kp_rows"], p["dof"], p["T"])


def columns_to_AB(p, cols, b, abi=False):
    """A, B of trajectory b, zero except at the key-points, from columns [entries][3][n] (kind 0 / 1 / 2 = column d of A, d + dof of A,
    d of B for d < m).  abi=False: the maths layout of oracle/crosscheck.py, A [T][row][col], B [T][row][m]; abi=True: the ABI's and the
    C oracle's column-major matrices, A [T][col][row], B [T][m][row]."""
    dof, n, m, T = p["dof"], p["n"], p["m"], p["T"]
    offs, times = entry_csr(p)
    A = np.zeros((T, n, n)); B = np.zeros((T, m, n) if abi else (T, n, m))
    for d in range(dof):
        e0, e1 = int(offs[b * dof + d]), int(offs[b * dof + d + 1])
        ts = times[e0:e1]
        for kind, c in ((0, d), (1, d + dof)):
            if abi: A[ts, c, :] = cols[e0:e1, kind]
            else: A[ts, :, c] = cols[e0:e1, kind]
        if d < m:
            if abi: B[ts, d, :] = cols[e0:e1, 2]
            else: B[ts, :, d] = cols[e0:e1, 2]
    return A, B


def oracle_on_columns(p, cols, b, lam, pd_stride=100):
    """The C oracle's a4 + a6 + a7 on the given key-point columns: dict(A, B, status, K, k, delta_J) in the ABI's layout"""
    n, m, nr, T, dof = p["n"], p["m"], p["nr"], p["T"], p["dof"]
    A, B = columns_to_AB(p, cols, b, abi=True)
    offs, c = p["kp_rows"][b]
    orc.interpolate(dof, m, T, offs, c, A, B)
    l_x, l_xx, l_u, l_uu = orc.cost_derivs(n, m, nr, T, p["r"][b], p["r_x"][b], p["r_u"][b], p["w_run"], p["w_term"])
    st, K, k, dJ = orc.backward(n, m, T, A, B, l_x, l_xx, l_u, l_uu, lam, pd_stride)
    return dict(A=A, B=B, status=st, K=K, k=k, delta_J=dJ)
