"""The blockwise measure of parity, and the graded problems on which it bites.

Every other parity test of the suite measures max|a - b| / max|b| over one trajectory's whole array: the bar is set by the
trajectory's single largest gain, and a control row or a state column of K that is small beside it -- a weak actuator, a weakly
coupled DoF, a step where the feed-forward is small -- can be wrong in its leading digits unseen.  Here the unit is the block:

    K_step   K_t                          k_step   k_t
    K_row    one control's row of K_t     U_step   the controls of one (alpha, step)
    K_col    one state's column of K_t    cost     the predicted cost of one alpha

and the error of a block is max|got - ref| over the block / max|ref| over the block.  A block whose reference is exactly zero is
held absolutely, to ZERO_ABS x the trajectory's largest entry of that array (the global measure's bar).

The reference is oracle/extended.py: the sweeps in longdouble on the oracle's A, B, l_*.  The bar of a block family on a given
trajectory is FACTOR[family] x the larger of the two CPU float64 implementations' own worst blockwise error against that
reference (the C oracle's and oracle/crosscheck.py's np_pipeline), floored at 1e-15 and capped at 1e-9: a float64 sweep is asked
to be as good, block by block, as the float64 sweeps we can read -- never as good as a GPU result happened to be."""
import hashlib

import numpy as np

import _shapes as S

from oracle import crosscheck as cc
from oracle import extended
from oracle import pipeline
from trajoptkp_amd import synth

FAMILIES = ("K_step", "K_row", "K_col", "k_step", "U_step", "cost")
# bar = FACTOR x max(oracle's own, np_pipeline's own, FLOOR), never above CAP.  32: the precedent of tests/_refresh.py (rho held to
# 32 x the oracle's own).  A family's factor is raised only on the evidence profiles/blockwise_parity.txt records.
FACTOR = {f: 32.0 for f in FAMILIES}
# cost: 64.  The oracle and np_pipeline add the T terms of a predicted cost in the same order, so their two errors are one sample
# of what the order of summation does, not two; the sweeps score steps in pairs and in tiles.  Shape suite, one-wave fused forward
# on per-DoF lists, dof 6, m 3, nr 1, T 17, trajectory 1 (profiles/blockwise_parity.txt): the GPU's worst predicted cost is 4.9e-14
# from the extended reference, the oracle's 1.3e-15 -- 36 times the oracle's own, rounding of another order of summation.
FACTOR["cost"] = 64.0
FLOOR, CAP, ZERO_ABS = 1e-15, 1e-9, 1e-9
LD = np.longdouble


def _blocks(x, axes):
    """max|x| over `axes` of every block."""
    return np.max(np.abs(x), axis=axes) if x.ndim else np.abs(x)


def _family_arrays(d):
    """family -> (array, the axes one block spans).  K [T][n][m] (column-major per step: K[t, state, control])."""
    return {"K_step": (d["K"], (1, 2)), "K_row": (d["K"], (1,)), "K_col": (d["K"], (2,)), "k_step": (d["k"], (1,)),
            "U_step": (d["U_alpha"], (2,)), "cost": (d["cost_pred"], ())}


def block_errors(got, ref):
    """got, ref: dicts with K [T][n][m], k [T][m], U_alpha [n_alpha][T][m], cost_pred [n_alpha] of ONE trajectory.  Returns
    {family: worst relative error over the blocks whose reference maximum is nonzero}, with two further keys per family:
    family + ":zero" the number of blocks whose reference is exactly zero and family + ":zero_abs" the worst max|got| over those
    blocks relative to the largest entry of the whole reference array."""
    out = {}
    fg, fr = _family_arrays(got), _family_arrays(ref)
    for f in FAMILIES:
        (g, axes), (r, _) = fg[f], fr[f]
        g, r = np.asarray(g, LD), np.asarray(r, LD)
        assert g.shape == r.shape, (f, g.shape, r.shape)
        diff = np.atleast_1d(_blocks(g - r, axes) if axes else np.abs(g - r))
        size = np.atleast_1d(_blocks(r, axes) if axes else np.abs(r))
        nz = size > 0
        out[f] = float(np.max(diff[nz] / size[nz])) if np.any(nz) else 0.0
        out[f + ":zero"] = int(np.sum(~nz))
        top = float(np.max(size)) if size.size else 0.0
        out[f + ":zero_abs"] = float(np.max(diff[~nz])) / max(top, 1e-300) if np.any(~nz) else 0.0
    return out


def violations(errs, bar):
    """The families of a block_errors result over their bar (or, in their exactly-zero blocks, over ZERO_ABS): [] passes."""
    bad = [(f, errs[f], bar[f]) for f in FAMILIES if not errs[f] <= bar[f]]
    return bad + [(f + ":zero_abs", errs[f + ":zero_abs"], ZERO_ABS) for f in FAMILIES if not errs[f + ":zero_abs"] <= ZERO_ABS]


def relerr(a, b):
    """The measure of the rest of the suite: the largest error over the largest entry."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def _fingerprint(p, b, lam, n_alpha, pd_stride):
    h = hashlib.blake2b(digest_size=16)
    sel = p["job_b"] == b
    offs, cols = p["kp_rows"][b]
    for x in (p["xplus"][sel], p["xminus"][sel], p["job_t"][sel], p["job_col"][sel], p["job_mode"][sel], p["xnom"][p["job_nom"][sel]],
              p["r"][b], p["r_x"][b], p["r_u"][b], p["u_nom"][b], p["w_run"], p["w_term"], p["ctrl_lim"], offs, cols):
        h.update(np.ascontiguousarray(x).tobytes())
    h.update(repr((p["n"], p["m"], p["nr"], p["T"], float(p["eps"]), float(lam), int(n_alpha), int(pd_stride))).encode())
    return h.digest()


_BARS = {}


def bars(p, b, lam=None, n_alpha=6, pd_stride=100):
    """The oracle, np_pipeline and the extended reference of trajectory b, on the CPU only.  Returns a dict: status (the oracle's;
    nothing else where it is not 0), ref (extended.extended_trajectory), oracle (pipeline.run_trajectory, want_U), own
    {"oracle" | "np": block_errors against ref} and bar {family: min(CAP, FACTOR x max(both own errors, FLOOR))}.  Cached per
    distinct trajectory (a fingerprint of its inputs): the shape, fuzz and blockwise suites share problems."""
    lam = p["lam"] if lam is None else lam
    key = _fingerprint(p, b, lam, n_alpha, pd_stride)
    if key in _BARS:
        return _BARS[key]
    o = pipeline.run_trajectory(p, b, lam=lam, pd_stride=pd_stride, n_alpha=n_alpha, want_U=True)
    out = dict(status=o["status"], oracle=o)
    if o["status"] == 0:
        ref = extended.extended_trajectory(p, b, lam, n_alpha, pd_stride)
        q = cc.np_pipeline(p, b, lam=lam, pd_stride=pd_stride, n_alpha=n_alpha)
        assert ref["status"] == 0 and q["status"] == 0, (ref["status"], q["status"])
        q = dict(K=cc._T(q["K"]), k=q["k"], U_alpha=q["U_alpha"], cost_pred=q["cost_pred"])
        own = {"oracle": block_errors(o, ref), "np": block_errors(q, ref)}
        bar = {f: min(CAP, FACTOR[f] * max(own["oracle"][f], own["np"][f], FLOOR)) for f in FAMILIES}
        out.update(ref=ref, np=q, own=own, bar=bar)
    _BARS[key] = out
    return out


def gpu_result(g, b):
    """Trajectory b of a GPU result of tests/_shape_run._run (K, k, cost, U over the batch) in block_errors' form."""
    return dict(K=g["K"][b], k=g["k"][b], U_alpha=g["U"][b], cost_pred=g["cost"][b])


def check(got, p, b, tag, lam=None, n_alpha=6, pd_stride=100):
    """Asserts one trajectory's result (block_errors' form) against the bars of trajectory b of p; returns (errs, the bars dict)."""
    bb = bars(p, b, lam, n_alpha, pd_stride)
    assert bb["status"] == 0, (tag, b, bb["status"])
    errs = block_errors(got, bb["ref"])
    bad = violations(errs, bb["bar"])
    assert not bad, (tag, b, bad, {f: errs[f] for f in FAMILIES}, bb["bar"])
    return errs, bb


# ---- graded problems ----------------------------------------------------------------------------------------------------
DECADES = 6.0
# The step of the graded copy's finite differences.  synth's 1e-6 leaves a differenced column an absolute noise of ulp(x) / 2 eps =
# 1e-10, and a column of B in a unit of 1e-6 (entries of 2e-9) would be that noise.  A step of 0.3 leaves 4e-16.
GRADED_EPS = 0.3
# The nominal controls of the copy, as a share of synth's (30 % of the limits).  u - u_nom is formed in float64 by every
# implementation; against a nominal value 1e12 units large its rounding, times l_u, is a fixed 4e-17 a term beside predicted costs
# that shrink with the controls' authority, and at synth's share the cost bars of one case in seven came out above 1e-10.
U_NOM_SHRINK = 2.0 ** -7


def _coprime_stride(n):
    k = 3
    while np.gcd(k, n) != 1:
        k += 2
    return k


def _geometric(count, decades, order=None):
    """count factors from 1 down to 10^-decades, geometrically; order: a permutation of their positions."""
    g = 10.0 ** (-decades * np.arange(count) / max(count - 1, 1))
    return g if order is None else g[np.asarray(order)]


def graded(p, decades=DECADES):
    """A copy of a synth problem in graded units, synth itself untouched.  Control j at step t is measured in a unit 1 / (s_j g_t):
    column j of B_t and of r_u times s_j g_t, its limits and nominal values over it.  State i is measured in a unit 1 / d_i (A -> D A
    D^-1, B -> D B, r_x -> r_x D^-1), and residual i is weighted a further w_i.  s, d, w and g (over the horizon) are each spread
    geometrically over `decades` decades, d interleaved so that neighbouring states are decades apart in both halves of the state.
    With lambda = 0 the gains of the copy would be the original's with rows and columns rescaled; under the fixed lambda it is a
    different, equally legitimate problem whose K_t has rows, columns and steps many decades apart, and whose k_t falls over the
    horizon -- the setting in which lanes, chunks, tiles and steps can be confused without the largest gain noticing.  The
    finite-difference payload is rebuilt about its nominal next states (one-sided jobs stay one-sided), so every upload form carries
    the copy; interpolation between key-points, cost derivatives and the sweeps then see it like any other problem.
    The drift g is there because units and weights alone leave K_t and k_t within two or three decades from step to step: with one
    control there is one row a step, and a row or a k_t wrong by 1e-6 of itself then shows at 1e-8 under the global measure too --
    tests/test_blockwise_model.py asks for errors that it does not see, on every case."""
    n, m, nr, T = p["n"], p["m"], p["nr"], p["T"]
    s = _geometric(m, decades) if m > 1 else np.ones(1)
    d = _geometric(n, decades, order=(np.arange(n) * _coprime_stride(n)) % n)
    w = _geometric(nr, decades) if nr > 1 else np.ones(1)
    g = _geometric(T, decades)
    q = dict(p)
    col = p["job_col"].astype(np.int64)
    is_b = col >= n
    unit = np.where(is_b, s[np.where(is_b, col - n, 0)] * g[p["job_t"]], 1.0 / d[np.where(is_b, 0, col)])   # of the perturbed column
    scale = unit[:, None] * d[None, :]
    x0 = p["xnom"][p["job_nom"]]
    mode = p["job_mode"][:, None]
    J = np.where(mode == 0, (p["xplus"] - p["xminus"]) / (2 * p["eps"]),
                 np.where(mode == 1, (p["xplus"] - x0) / p["eps"], (x0 - p["xminus"]) / p["eps"])) * scale
    q["eps"] = GRADED_EPS
    q["xplus"] = np.where(mode == 2, x0, x0 + GRADED_EPS * J)
    q["xminus"] = np.where(mode == 1, x0, x0 - GRADED_EPS * J)
    q["r_x"] = p["r_x"] / d[None, None, None, :]
    q["r_u"] = p["r_u"] * s[None, None, None, :] * np.append(g, g[-1])[None, :, None, None]
    q["rx_const"] = None if p.get("rx_const") is None else p["rx_const"] / d[None, :]
    q["w_run"], q["w_term"] = p["w_run"] * w, p["w_term"] * w
    q["u_nom"] = U_NOM_SHRINK * p["u_nom"] / s[None, None, :] / g[None, :, None]
    q["ctrl_lim"] = p["ctrl_lim"] / np.repeat(s, 2) / g[-1]
    for key in ("A_kp", "B_kp"):                            # (what synth drew the payload from; no stage reads them)
        q.pop(key, None)
    return q


def problem(c):
    """The graded problem of a case: two or three distinct trajectories, tiled up to the case's batch where that is larger."""
    from _shape_run import _problem, _take
    base = graded(_problem(c, batch=min(c["batch"], 3)))
    if c["batch"] <= 3:
        return base, base
    return base, _take(synth.tile_problem(base, -(-c["batch"] // 3)), c["batch"])


# ---- the cases of tests/test_gpu_blockwise.py -----------------------------------------------------------------------------
def family(c):
    """The kernel family whose table a case belongs to: one_tile (the four one-tile shapes, fused or not), tiled, wide, generic."""
    bv = S.select_variants(c["dof"], c["m"], c["nr"], c["T"], c["n_alpha"], c["batch"], c["flags"], c["env"])[0]
    return {"mfma_f64_t1": "one_tile", "mfma_f64_t1_fused": "one_tile", "mfma_f64_tiled": "tiled", "mfma_f64_tiled_a6": "tiled",
            "mfma_f64_wide": "wide", "generic_lds": "generic"}[bv]


def cases(n_simd):
    """The cases of tests/test_gpu_blockwise.py, each run on the graded copy of its problem (T = 17, two distinct trajectories):
      - the tiled sweeps at two, three and four state tiles with m = 1, 7, 8, the wide sweeps at two, three and four with m = 9, 17,
        32 and the generic sweeps, by hand;
      - a cover of every other key of _shapes.COMPILED drawn from the shape suite's own table (tests/_shapes.py: its T = 17 cases,
        and the n_simd + 1 batches of batch_cases for the `plain` kernels), chosen greedily in the table's order: the fewest cases
        that still reach every instantiation, all four one-tile shapes among them in every fused and unfused form;
      - one T = 131 case per family (the Newton-Schulz refresh and the PD stride crossed)."""
    out = [S._case(dof, m, 4, S.FLAG_TILED, why="graded_tiled") for dof in (9, 19, 27) for m in (1, 7, 8)]
    out += [S._case(dof, m, 5, 0, why="graded_wide") for dof in (12, 20, 28) for m in (9, 17, 32)]
    out += [S._case(7, 7, 4, S.FLAG_GENERIC, why="graded_generic"), S._case(32, 7, 4, 0, why="graded_generic")]
    pool = [c for c in S.cases(n_simd) if c["why"] not in ("refused", "long", "n_alpha") and c["T"] == 17]
    pool += [dict(c, T=17) for c in S.batch_cases(n_simd) if c["batch"] == n_simd + 1]
    left = set(S.COMPILED)
    for c in out:
        left.difference_update(S.case_keys(c, n_simd))
    while left:
        gain = [len(left.intersection(S.case_keys(c, n_simd))) for c in pool]
        best = int(np.argmax(gain))
        assert gain[best] > 0, sorted(left)
        out.append(pool[best])
        left.difference_update(S.case_keys(pool[best], n_simd))
    one_wave = {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}
    for dof, m, flags, env in ((7, 7, S.FLAG_FUSED, one_wave), (7, 7, S.FLAG_FUSED, {}), (7, 7, 0, {}), (14, 5, S.FLAG_TILED, {}),
                               (21, 8, S.FLAG_FUSED, S.TILED_ENVS["a6"]), (16, 17, 0, {}), (7, 7, S.FLAG_GENERIC, {})):
        out.append(S._case(dof, m, 4, flags, env, T=131, rx_const=bool(flags & S.FLAG_FUSED), why="graded_long"))
    return out
