"""KPILQR_FLAG_EMBED_SHAPE restated in Python: the choice of the carrier shape (kp_t1_carrier, mfma_common.h, with the bounds
choose_embedding adds in kpilqr_api.cpp), the expansion of the caller's per-DoF key-point CSR to the carrier's (kpilqr_set_keypoints
on an embedded context), and the zero-padding of a synth problem into the carrier's dims ON THE HOST -- what a context created
natively at the carrier's shape has to be fed to see the bits the embedding kernels (embed.hip) produce on the device.

tests/test_embed_model.py checks this model against itself and against the CPU oracle (no GPU); tests/test_gpu_embed.py runs it
against the library."""
import numpy as np

import _shapes as S
from trajoptkp_amd import synth
from trajoptkp_amd.engine import rows_to_dof_csr

FLAG_EMBED = 16                                         # KPILQR_FLAG_EMBED_SHAPE, include/kpilqr.h


def carrier(dof, m):
    """(dof', m') of the compiled shape with the smallest n', then the smallest m', that contains (dof, m); a compiled shape is its
    own carrier; None where m > dof or nothing contains the shape."""
    if dof < 1 or m < 1 or m > dof:
        return None
    fits = sorted((n, mm) for n, mm in S.T1_SHAPES if 2 * dof <= n and m <= mm)
    return (fits[0][0] // 2, fits[0][1]) if fits else None


def embedded(dof, m, nr, T, n_alpha, flags):
    """The carrier (dof', m') a context of these dims and flags is embedded into, or None where the flag is ignored: not set,
    FUSED missing, GENERIC / TILED forced, a shape with its own instantiation, no carrier, or the fused sweeps' own bounds
    (fused_supported) missed at the carrier's dims."""
    if not flags & FLAG_EMBED or not flags & S.FLAG_FUSED or flags & (S.FLAG_GENERIC | S.FLAG_TILED):
        return None
    if (2 * dof, m) in S.T1_SHAPES:
        return None
    c = carrier(dof, m)
    if c is None or not S.fused_supported(2 * c[0], c[1], nr, c[0], T, n_alpha):
        return None
    return c


def row_map(dof, cdof):
    """Carrier row of every state row (and r_x column) of the caller: i < dof -> i, i >= dof -> i + (dof' - dof)."""
    i = np.arange(2 * dof)
    return np.where(i < dof, i, i + (cdof - dof))


def expand_csr(offs, times, batch, dof, cdof):
    """The caller's per-DoF CSR (batch * dof lists) -> the carrier's (batch * dof' lists): the caller's lists d < dof, then
    dof' - dof copies of the trajectory's list 0."""
    offs = np.asarray(offs); times = np.asarray(times)
    out_o, out_t = [0], []
    for b in range(batch):
        for d in range(cdof):
            l = b * dof + (d if d < dof else 0)
            out_t.append(times[offs[l]:offs[l + 1]])
            out_o.append(out_o[-1] + len(out_t[-1]))
    return np.asarray(out_o, np.int32), (np.concatenate(out_t).astype(np.int32) if out_t else np.zeros(0, np.int32))


def pad_problem(p, cdof, cm):
    """A synth problem zero-embedded into (dof', m') = (cdof, cm) on the host: padded states get zero A columns and rows, zero B
    rows and zero r_x columns (no FD job perturbs a padded DoF, and every x+ / x- row is +0 there), padded controls zero B columns
    (no job), zero r_u columns, zero nominal controls and the limits (-1, 1).  The padded DoFs' key-point lists are copies of the
    trajectory's list 0.  Residuals, weights, eps and lambda are shape-free."""
    dof, n, m, T, B = p["dof"], p["n"], p["m"], p["T"], p["batch"]
    assert dof <= cdof and m <= cm
    cn, rm = 2 * cdof, row_map(dof, cdof)
    q = dict(p)
    q.update(dof=cdof, n=cn, m=cm)
    q.pop("A_kp", None); q.pop("B_kp", None)
    col = p["job_col"].astype(np.int64)
    q["job_col"] = np.where(col < n, rm[np.minimum(col, n - 1)], cn + (col - n)).astype(np.int32)

    def rows(x):
        out = np.zeros(x.shape[:-1] + (cn,))
        out[..., rm] = x
        return out

    def ctrl(x, fill=0.0):
        out = np.full(x.shape[:-1] + (cm,), fill)
        out[..., :m] = x
        return out
    for key in ("xplus", "xminus", "xnom"):
        q[key] = rows(p[key])
    q["r_x"] = rows(p["r_x"])
    q["r_u"] = ctrl(p["r_u"])
    q["u_nom"] = ctrl(p["u_nom"])
    lim = np.tile(np.array([-1.0, 1.0]), cm)
    lim[:2 * m] = p["ctrl_lim"]
    q["ctrl_lim"] = lim
    q["rx_const"] = None if p.get("rx_const") is None else rows(p["rx_const"])
    o, t = rows_to_dof_csr(p["kp_rows"], dof, T)
    eo, et = expand_csr(o, t, B, dof, cdof)
    q["kp_rows"] = [synth.rows_from_dof_lists(cdof, T, [et[eo[b * cdof + d]:eo[b * cdof + d + 1]] for d in range(cdof)])
                    for b in range(B)]
    q["kp_times"] = None
    return q


def real_block(res, dof, m, cdof):
    """The caller's block of results computed at the carrier's shape (K [..., n', m'], k / U [..., m']), and what is left of K and
    k outside it (the padded gains)."""
    rm = row_map(dof, cdof)
    out = dict(res)
    K = np.asarray(res["K"])
    out["K"] = K[..., rm, :][..., :m]
    mask = np.ones(K.shape[-2:], bool)
    mask[np.ix_(rm, np.arange(m))] = False
    out["K_pad"] = K[..., mask]
    out["k"] = np.asarray(res["k"])[..., :m]
    out["k_pad"] = np.asarray(res["k"])[..., m:]
    for key in ("U", "U_alpha"):
        if res.get(key) is not None:
            out[key] = np.asarray(res[key])[..., :m]
    return out
