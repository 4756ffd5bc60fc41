"""Shared by tests/test_gpu_partial_sweeps.py: the cases (one per kernel body a listed launch can reach, built with _shapes._case), the
two problems of a case, and the protocol every case and list goes through.

Protocol.  Two problems p0 and p1 of one shape with the same key-point lists and different data (config ids 41 / 42).
  1. a context uploads p0 whole, runs the whole-batch backward and forward sweep: the SNAPSHOT of K, k, status, delta_J, cost_pred
  2. the listed rows of p1 go up through the existing partial calls, then the listed sweeps run with new lambdas (LAM1)
  yardstick 1: a fresh context of batch = count given p1's listed trajectories through the whole-batch calls, same environment:
               np.array_equal on every compact output and on the listed rows of the device buffers
  yardstick 2: every unlisted row of the device buffers np.array_equal the snapshot
  yardstick 3: the listed trajectories against oracle.pipeline.run_trajectory at _shape_run.RTOL, status exact
Everything computed here is computed once per process and never modified."""
import functools

import numpy as np

import _shape_run as R
import _shapes as S
from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import synth
from trajoptkp_amd.engine import rows_to_dof_csr

B, T = 5, 17
LISTS = {"first": [0], "last": [B - 1], "run": [1, 2, 3], "gaps": [0, 2, 4], "all": list(range(B)), "none": []}
ALPHAS = orc.alphas(6)
LAM1 = np.array([0.3, 0.05, 0.7, 0.02, 0.15])          # the lambdas of step 2, one per trajectory (p0 runs at its own 0.1)
PER_TRAJ = ("r", "r_x", "r_u", "u_nom")
JOBS = ("job_b", "job_t", "job_col", "job_mode", "job_nom", "xplus", "xminus")
ONE_WAVE = {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}
F = S.FLAG_FUSED


def _c(dof, m, nr, flags, env=None, T=T, **kw):
    return S._case(dof, m, nr, flags, env, T=T, batch=B, why="partial_sweeps", **kw)


# name: (case, what kpilqr_last_launch(backward) has to contain, ... (forward))
CASES = {
    "fused_w1_rxc": (_c(7, 7, 9, F, ONE_WAVE, rx_const=True), ":w1:kpc:uni", ":w1:uni"),
    "fused_pair_uni": (_c(7, 7, 4, F, {"KPILQR_FUSED_WAVES": "5", "KPILQR_FUSED_FWD_WAVES": "4"}), ":pairh:kpc:uni", ":pair:uni"),
    "fused_pair_triple_ragged": (_c(7, 7, 4, F, {"KPILQR_FUSED_WAVES": "5", "KPILQR_FUSED_FWD_WAVES": "3"}, uniform=False), ":pairh:kpc:ragged", ":triple:ragged"),
    "fused_w1_ragged_slopes": (_c(7, 7, 4, F, ONE_WAVE, uniform=False), ":w1:kpc:ragged", ":w1:ragged"),
    "fused_2_1": (_c(2, 1, 3, F, ONE_WAVE), ":w1:kpc:uni", ":w1:uni"),
    "t1": (_c(7, 7, 4, 0), "mfma_f64_t1", "mfma_f64_t1"),
    "tiled_uw": (_c(9, 7, 4, 0), "mfma_f64_tiled", "mfma_f64_tiled:state_cost_waves"),
    "tiled_col4": (_c(26, 7, 4, 0), "mfma_f64_tiled", "mfma_f64_tiled"),
    "tiled_a6": (_c(12, 7, 4, F, S.TILED_ENVS["a6"]), "mfma_f64_tiled_a6", "mfma_f64_tiled_a6"),
    "tiled_no_fsc": (_c(9, 7, 4, 0, S.TILED_ENVS["no_fsc"]), "mfma_f64_tiled", "mfma_f64_tiled"),
    "wide_m9": (_c(12, 9, 5, 0), "mfma_f64_wide", "mfma_f64_tiled"),
    "wide_m17": (_c(12, 17, 5, 0), "mfma_f64_wide", "mfma_f64_wide"),
    "generic": (_c(7, 7, 4, S.FLAG_GENERIC), "generic_lds", "generic_lds"),
}
LONG = {          # T = 131: the PD stride of 100 and the refresh are crossed
    "fused_w1_rxc_long": (_c(7, 7, 4, F, ONE_WAVE, T=131, rx_const=True), ":w1:kpc:uni", ":w1:uni"),
    "tiled_long": (_c(14, 5, 4, S.FLAG_TILED, T=131), "mfma_f64_tiled", "mfma_f64_tiled:state_cost_waves"),
}
# the one-wave fused sweeps on dense residuals: the problem of the PD-failure and retry tests (negative running weights, NEG_SCALE)
EXTRA = {"fused_w1": (_c(7, 7, 4, F, ONE_WAVE), ":w1:kpc:uni", ":w1:uni")}
ALL_CASES = dict(CASES, **LONG, **EXTRA)
# w_run = -(|w_run| + 1) * NEG_SCALE on `fused_w1`, pd_stride 10: on the oracle every trajectory of p0 and p1 fails its PD check for
# lambda <= 0.15 and passes for lambda >= 1 (between the two the outcome depends on the trajectory); the tests use lambdas a factor
# of three or more away from that band -- 0.03 and below to fail, 3 and above to settle -- and assert the oracle's statuses first.
NEG_SCALE, NEG_PD = 3.0, 10
LAM_FAIL, LAM_OK = 0.03, 3.0


def case_key(c):
    return R._case_id(c)


@functools.lru_cache(maxsize=None)
def pair(name, neg_scale=None):
    """(p0, p1) of a case.  neg_scale: negative running weights w_run = -(|w_run| + 1) * neg_scale, as tests/_lambda_retry.py makes
    sweeps fail their PD checks."""
    c = ALL_CASES[name][0]
    p0, p1 = R._problem(c, config_id=41), R._problem(c, config_id=42)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(p0["kp_rows"], p1["kp_rows"]))
    assert not np.array_equal(p0["r"], p1["r"]) and not np.array_equal(p0["xplus"], p1["xplus"])
    if c["rx_const"]:
        assert np.array_equal(p0["rx_const"], p1["rx_const"])
    if neg_scale is not None:
        for p in (p0, p1):
            p["w_run"] = -(np.abs(p["w_run"]) + 1.0) * neg_scale
    return p0, p1


def sub(p, who):
    """The trajectories `who` (increasing) of a problem as a problem of their own, in list order."""
    who = [int(b) for b in who]
    q = dict(p)
    sel = np.isin(p["job_b"], who)
    for k in JOBS:
        q[k] = p[k][sel]
    q["job_b"] = np.searchsorted(np.asarray(who), q["job_b"]).astype(np.int32)
    for k in PER_TRAJ:
        q[k] = p[k][who]
    q["kp_rows"] = [p["kp_rows"][b] for b in who]
    q["batch"] = len(who)
    return q


def entries_of(p, traj):
    o, _ = rows_to_dof_csr(p["kp_rows"], p["dof"], p["T"])
    dof = p["dof"]
    return np.concatenate([np.arange(o[b * dof], o[(b + 1) * dof]) for b in traj]) if len(traj) else np.zeros(0, np.int64)


def is_fused(e):
    return e.backward_variant == "mfma_f64_t1_fused"


def upload_listed(e, c, p1, who, linearise=True):
    """Step 2 of the protocol up to the sweeps: the listed rows of p1 through the existing partial calls.  A fused context: the lists
    again (the same ones: the ranges are pending, as behind any update), the key-point ordered records of the listed entries; a context
    with records: the listed trajectories' jobs, and -- linearise -- kpilqr_fd_interpolate_partial and kpilqr_cost_derivs_partial."""
    who = [int(b) for b in who]
    if not who:
        return
    if is_fused(e):
        e.update_keypoints_rows(who, [p1["kp_rows"][b] for b in who])
        xp, xm, md = synth.kp_ordered_payload(p1)
        idx = entries_of(p1, who)
        e.upload_fd_kp_partial(who, e.fd_kp_slab(xp[idx], xm[idx], md[idx]), eps=p1["eps"])
    else:
        s = np.isin(p1["job_b"], who)
        e.upload_fd(p1["job_b"][s], p1["job_t"][s], p1["job_col"][s], p1["job_mode"][s], p1["xplus"][s], p1["xminus"][s],
                    job_nom=p1["job_nom"][s], xnom=p1["xnom"], eps=p1["eps"])
    if c["rx_const"]:
        e.upload_residuals_partial(who, p1["r"][who])
    else:
        e.upload_residuals_partial(who, p1["r"][who], p1["r_x"][who], p1["r_u"][who] if np.any(p1["r_u"]) else None)
    e.upload_nominal_partial(who, p1["u_nom"][who])
    if linearise and not is_fused(e):
        e.fd_interpolate_partial(who)
        if not e.backward_variant.endswith("_a6"):
            e.cost_derivs_partial(who)


def snapshot(e):
    """The device buffers a sweep writes: K, k, status, delta_J, cost_pred."""
    K, k = e.gains()
    res = e.results()
    return dict(K=K, k=k, status=res["status"], delta_J=res["delta_J"], cost=res["cost_pred"])


def whole(e, c, p, lam, pd=100):
    """Upload p whole, the stages the family needs, the whole-batch backward and forward sweep (lam: [batch])."""
    q = dict(p); q["lam"] = np.asarray(lam, float)
    st, dJ = R._backward(e, c, q, kp_ordered=True, pd=pd)
    cost, U = e.forward_linear(ALPHAS, want_U=True)
    return dict(status=st, delta_J=dJ, cost=cost, U=U)


@functools.lru_cache(maxsize=None)
def oracle(name, which, b, lam, pd=100, neg_scale=None):
    return pipeline.run_trajectory(pair(name, neg_scale)[which], b, lam=lam, pd_stride=pd, want_U=True)


def run_protocol(name, who, monkeypatch, pd=100, iterate=False, lam1=LAM1, neg_scale=None, lam0=None, retry=None):
    """-> dict(snap, after, got, fresh, launch, retry_got, retry_fresh).  got: the compact outputs of the listed calls; fresh: outputs
    and buffers of the fresh context of the listed trajectories (None for an empty list)."""
    c = ALL_CASES[name][0]
    p0, p1 = pair(name, neg_scale)
    who = np.asarray(list(who), dtype=np.int64)          # (an index array: an empty list indexes nothing)
    lam0 = np.full(B, p0["lam"]) if lam0 is None else np.asarray(lam0, float)
    lam1 = np.asarray(lam1, float)
    R._set_env(c, monkeypatch)
    out = {}
    with R._engine(c, p0) as e:
        if retry:
            e.set_lambda_retry(**retry)
        whole(e, c, p0, lam0, pd)
        out["snap"] = snapshot(e)
        if retry:
            out["retry_snap"] = e.lambda_retry()
        upload_listed(e, c, p1, who, linearise=not iterate)
        if iterate:
            e.iterate_partial(who, lam1[who], pd, ALPHAS)
            res = e.results()
            out["got"] = dict(status=res["status"][who], delta_J=res["delta_J"][who], cost=res["cost_pred"][who])
        else:
            st, dJ = e.backward_partial(who, lam1[who], pd)
            cost, U = e.forward_linear_partial(who, ALPHAS, want_U=True)
            out["got"] = dict(status=st, delta_J=dJ, cost=cost, U=U)
        out["after"] = snapshot(e)
        if retry:
            out["retry_after"] = e.lambda_retry()
        out["launch"] = (e.last_launch("backward"), e.last_launch("forward"), e.last_launch("linearise"))
    out["fresh"] = None
    if len(who):
        q = sub(p1, who)
        with R._engine(c, q) as e:
            if retry:
                e.set_lambda_retry(**retry)
            f = whole(e, c, q, lam1[who], pd)
            f.update({"buf_" + k: v for k, v in snapshot(e).items()})
            if retry:
                out["retry_fresh"] = e.lambda_retry()
            out["fresh"] = f
    return out


def check_protocol(name, who, out, pd=100, lam1=LAM1, neg_scale=None, iterate=False):
    """The three yardsticks and the launch strings."""
    c, want_b, want_f = ALL_CASES[name]
    who = np.asarray(list(who), dtype=np.int64)
    rest = np.asarray([b for b in range(B) if b not in who], dtype=np.int64)
    snap, after, got, fresh = out["snap"], out["after"], out["got"], out["fresh"]
    assert np.any(snap["K"] != 0) and np.any(snap["cost"] != 0)
    for key in snap:                                               # yardstick 2: nobody else's bytes
        assert np.array_equal(after[key][rest], snap[key][rest]), (name, who, key, "unlisted rows changed")
    if not len(who):
        assert not any(x.endswith(":subset") for x in out["launch"][:2]), out["launch"]
        return
    # yardstick 1.  The status of every listed trajectory; everything else of those whose sweep settled: a sweep that fails its PD
    # check stops there, in a listed launch as in a whole-batch one, and the steps it did not reach keep what they held -- the
    # snapshot's gains here, zeros in the fresh context -- so a failed trajectory's gains and predictions are nobody's yardstick.
    assert np.array_equal(got["status"], fresh["status"]) and np.array_equal(after["status"][who], fresh["buf_status"]), (name, who, "status")
    ok = np.flatnonzero(fresh["status"] == 0)
    for key in ("delta_J", "cost") + (() if iterate else ("U",)):                  # compact outputs ...
        assert np.array_equal(got[key][ok], fresh[key][ok]), (name, who, key, "compact output differs from the fresh context's")
    for key in snap:                                               # ... and the listed rows of the device buffers
        assert np.array_equal(after[key][who[ok]], fresh["buf_" + key][ok]), (name, who, key, "listed rows differ from the fresh context's")
    assert not np.array_equal(after["K"][who], snap["K"][who])
    for i, b in enumerate(who):                                    # yardstick 3
        o = oracle(name, 1, b, float(lam1[b]), pd, neg_scale)
        assert got["status"][i] == o["status"], (name, b, got["status"][i], o["status"])
        if o["status"] != 0:
            continue
        errs = dict(K=R._rel(after["K"][b], o["K"]), k=R._rel(after["k"][b], o["k"]),
                    delta_J=abs(got["delta_J"][i] - o["delta_J"]) / max(abs(o["delta_J"]), 1e-300), cost=R._rel(got["cost"][i], o["cost_pred"]))
        if not iterate:
            errs["U"] = R._rel(got["U"][i], o["U_alpha"])
        assert max(errs.values()) <= R.RTOL, (name, b, errs)
    lb, lf, ll = out["launch"]
    assert want_b in lb and lb.endswith(":subset"), (lb, want_b)
    assert want_f in lf and lf.endswith(":subset"), (lf, want_f)
    if "state_cost_waves" not in want_f:
        assert "state_cost_waves" not in lf, lf
    if "slopes" in name:
        assert ":slopes" in lb and ":slopes" in lf, (lb, lf)
    if "rxc" in name:
        assert ":rxc" in lb and ":rxc" in lf, (lb, lf)
