"""GPU tests of the sweeps over a listed subset of the batch: kpilqr_backward_partial, kpilqr_forward_linear_partial and
kpilqr_iterate_partial (include/kpilqr.h, "Sweeps of a subset").  tests/_partial_sweeps.py holds the cases -- one per kernel body a
listed launch can reach -- and the protocol: a snapshot of a whole-batch run on p0, the listed rows of p1 through the existing partial
calls, the listed sweeps with new lambdas, then three yardsticks: a fresh context of exactly the listed trajectories (bit for bit),
the snapshot for every unlisted row (bit for bit), the oracle (1e-9, status exact).  B = 5, T = 17."""
import ctypes as C

import numpy as np
import pytest

import _partial_sweeps as P
import _shape_run as R
import _shapes as S
from oracle import pipeline
from trajoptkp_amd import _lib, synth
from trajoptkp_amd.engine import KpilqrError

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -5
LIST_IDS = list(P.LISTS)


# ---- 1. every kernel body, every list -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", LIST_IDS)
@pytest.mark.parametrize("name", list(P.CASES))
def test_listed_sweeps(name, subset, monkeypatch):
    who = P.LISTS[subset]
    P.check_protocol(name, who, P.run_protocol(name, who, monkeypatch))


@pytest.mark.parametrize("subset", ["gaps", "run"])
@pytest.mark.parametrize("name", list(P.LONG))
def test_listed_sweeps_across_the_pd_stride_and_the_refresh(name, subset, monkeypatch):
    who = P.LISTS[subset]
    P.check_protocol(name, who, P.run_protocol(name, who, monkeypatch))


# ---- 2. the whole iteration ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", ["gaps", "last", "none"])
@pytest.mark.parametrize("name", ["fused_pair_uni", "tiled_uw", "t1"])
def test_iterate_partial(name, subset, monkeypatch):
    who = P.LISTS[subset]
    out = P.run_protocol(name, who, monkeypatch, iterate=True)
    P.check_protocol(name, who, out, iterate=True)
    if who:
        fused = name.startswith("fused")
        assert out["launch"][2] == ("in_sweep:subset" if fused else "fd_difference+interpolate:subset"), out["launch"]


# ---- 3. PD failures -----------------------------------------------------------------------------------------------------------
def test_a_failing_listed_and_a_failing_unlisted_trajectory(monkeypatch):
    """Negative running weights (tests/_partial_sweeps.py, NEG_SCALE): trajectory 1 fails in step 1 and is not listed, trajectory 0
    is listed and fails at its new lambda.  The listed status is the fresh context's, the unlisted one the snapshot's."""
    who = [0, 2, 4]
    lam0 = np.array([30.0, P.LAM_FAIL, 30.0, 30.0, 30.0])
    lam1 = np.array([P.LAM_FAIL, 30.0, P.LAM_OK, 30.0, 30.0])
    assert P.oracle("fused_w1", 0, 1, P.LAM_FAIL, P.NEG_PD, P.NEG_SCALE)["status"] != 0
    assert [P.oracle("fused_w1", 1, b, float(lam1[b]), P.NEG_PD, P.NEG_SCALE)["status"] != 0 for b in who] == [True, False, False]
    out = P.run_protocol("fused_w1", who, monkeypatch, pd=P.NEG_PD, lam1=lam1, lam0=lam0, neg_scale=P.NEG_SCALE)
    assert out["snap"]["status"][1] != 0 and not np.any(out["snap"]["status"][[0, 2, 3, 4]])
    P.check_protocol("fused_w1", who, out, pd=P.NEG_PD, lam1=lam1, neg_scale=P.NEG_SCALE)
    assert out["got"]["status"][0] != 0 and not np.any(out["got"]["status"][1:])
    assert out["after"]["status"][1] == out["snap"]["status"][1] != 0


# ---- 4. the lambda retry schedule ---------------------------------------------------------------------------------------------
RETRY = dict(factor=100.0, max_lambda=1e4, max_attempts=3)


@pytest.mark.parametrize("who", [[0, 2, 4], [1]], ids=["gaps", "one"])
def test_lambda_retry_composes_with_a_list(who, monkeypatch):
    """Trajectory 3 starts step 1 at 3e-7: three failing attempts (3e-7, 3e-5, 3e-3), the schedule's maximum, and its resident status
    stays non-zero; it is never listed, so no listed call may arm it.  The first listed trajectory starts at LAM_FAIL and settles
    at its second attempt (LAM_FAIL * 100 = LAM_OK); the others settle at once."""
    lam0 = np.array([30.0, 30.0, 30.0, 3e-7, 30.0])
    lam1 = np.full(P.B, 30.0); lam1[who[0]] = P.LAM_FAIL
    for lam in (3e-7, 3e-5, 3e-3):
        assert P.oracle("fused_w1", 0, 3, lam, P.NEG_PD, P.NEG_SCALE)["status"] != 0
    assert P.oracle("fused_w1", 1, who[0], P.LAM_FAIL, P.NEG_PD, P.NEG_SCALE)["status"] != 0
    assert P.oracle("fused_w1", 1, who[0], P.LAM_FAIL * 100.0, P.NEG_PD, P.NEG_SCALE)["status"] == 0
    out = P.run_protocol("fused_w1", who, monkeypatch, pd=P.NEG_PD, lam1=lam1, lam0=lam0, neg_scale=P.NEG_SCALE, retry=RETRY)
    rest = [b for b in range(P.B) if b not in who]
    snap_lam, snap_att = out["retry_snap"]
    assert out["snap"]["status"][3] != 0 and snap_att[3] == 3 and snap_lam[3] == 3e-7 * 100.0 * 100.0
    # yardsticks 1 and 2 for every output, the retry outputs included
    lam_used, att = out["retry_after"]
    f_lam, f_att = out["retry_fresh"]
    assert np.array_equal(lam_used[who], f_lam) and np.array_equal(att[who], f_att)
    assert att[who[0]] == 2 and lam_used[who[0]] == P.LAM_FAIL * 100.0 and np.all(att[who[1:]] == 1)
    assert np.array_equal(lam_used[rest], snap_lam[rest]) and np.array_equal(att[rest], snap_att[rest])
    for key in out["snap"]:
        assert np.array_equal(out["after"][key][rest], out["snap"][key][rest]), key
        assert np.array_equal(out["after"][key][who], out["fresh"]["buf_" + key]), key
    for key in ("status", "delta_J", "cost", "U"):
        assert np.array_equal(out["got"][key], out["fresh"][key]), key
    assert not np.any(out["got"]["status"])
    # the oracle at the lambda each listed trajectory settled at
    for i, b in enumerate(who):
        o = P.oracle("fused_w1", 1, b, float(lam_used[b]), P.NEG_PD, P.NEG_SCALE)
        assert o["status"] == 0
        assert R._rel(out["after"]["K"][b], o["K"]) <= R.RTOL and R._rel(out["got"]["cost"][i], o["cost_pred"]) <= R.RTOL
    assert out["launch"][0].endswith(":subset")


def test_resident_lambdas_follow_the_list(monkeypatch):
    """lambda = NULL behind a listed call sweeps with what is resident: the new lambdas of the listed trajectories, everybody else's
    old ones.  A whole-batch sweep with the resident lambdas equals a fresh context's sweep of the merged problem at the merged lambdas."""
    name, who = "fused_w1_rxc", [0, 2, 4]
    c = P.ALL_CASES[name][0]
    p0, p1 = P.pair(name)
    lam0 = np.full(P.B, 0.1)
    merged_lam = lam0.copy(); merged_lam[who] = P.LAM1[who]
    R._set_env(c, monkeypatch)
    with R._engine(c, p0) as e:
        P.whole(e, c, p0, lam0)
        P.upload_listed(e, c, p1, who)
        e.backward_partial(who, P.LAM1[who])
        e.forward_linear_partial(who, P.ALPHAS)
        e.backward(None)                                   # the resident lambdas, the whole batch
        e.forward_linear(P.ALPHAS)
        got = P.snapshot(e)
        assert not e.last_launch("backward").endswith(":subset")
    pm = dict(p1)                                          # p1 for the listed trajectories, p0 elsewhere
    sel = np.zeros(P.B, bool); sel[who] = True
    for k in P.PER_TRAJ:
        pm[k] = np.where(sel.reshape((P.B,) + (1,) * (p0[k].ndim - 1)), p1[k], p0[k])
    pm["xnom"] = np.concatenate([p0["xnom"], p1["xnom"]])
    k0, k1 = ~sel[p0["job_b"]], sel[p1["job_b"]]
    for k in P.JOBS:
        pm[k] = np.concatenate([p0[k][k0], (p1[k][k1] + len(p0["xnom"])) if k == "job_nom" else p1[k][k1]])
    order = np.argsort(pm["job_b"], kind="stable")
    for k in P.JOBS:
        pm[k] = pm[k][order]
    with R._engine(c, pm) as e:
        P.whole(e, c, pm, merged_lam)
        want = P.snapshot(e)
    for key in want:
        assert np.array_equal(got[key], want[key]), key


# ---- 5. the form follows the count --------------------------------------------------------------------------------------------
def _rows8(batch):
    return sorted(set(int(x) for x in np.linspace(0, batch - 1, 8)))


@pytest.fixture(scope="module")
def tiled_base():
    c = S._case(7, 7, 9, S.FLAG_FUSED, batch=2, rx_const=True, why="form")
    p = R._problem(c)
    refs = [pipeline.run_trajectory(p, b, want_U=True) for b in range(2)]
    return c, p, refs


def _form_run(c, p, batch, counts, monkeypatch):
    """One context of `batch` trajectories (the two of p, tiled): the whole-batch sweeps, then for every count a listed sweep over
    the FIRST trajectories but one and the last (a list that is no prefix).  -> [(launch strings, K, cost of eight spread rows)]"""
    q = synth.tile_problem(p, (batch + 1) // 2)
    q = R._take(q, batch) if q["batch"] != batch else q
    cc = dict(c, batch=batch)
    R._set_env(cc, monkeypatch)
    out = []
    with R._engine(cc, q) as e:
        P.whole(e, cc, q, np.full(batch, p["lam"]))
        rows = _rows8(batch)
        Kw, _ = e.gains(traj=rows, want_k=False)
        out.append(((e.last_launch("backward"), e.last_launch("forward")), rows, Kw, e.results()["cost_pred"][rows]))
        for count in counts:
            who = list(range(count - 1)) + [batch - 1] if count < batch else list(range(batch))
            st, _ = e.backward_partial(who, p["lam"])
            cost = e.forward_linear_partial(who, P.ALPHAS)
            assert not np.any(st)
            pick = sorted(set(int(x) for x in np.linspace(0, count - 1, 8)))
            rows_l = [who[i] for i in pick]
            Kl, _ = e.gains(traj=rows_l, want_k=False)
            out.append(((e.last_launch("backward"), e.last_launch("forward")), rows_l, Kl, cost[pick]))
    return out


def _hold(out, refs):
    """eight spread rows of every launch against the oracle and against the whole-batch sweep, 1e-9 (the form differs: not bit for bit)"""
    (_, rows_w, Kw, cw) = out[0]
    of_parity = {b % 2: i for i, b in enumerate(rows_w)}          # (the batch is two trajectories, tiled)
    assert set(of_parity) == {0, 1}
    for (launch, rows, K, cost) in out:
        assert len(rows) == 8
        for i, b in enumerate(rows):
            o = refs[b % 2]
            assert R._rel(K[i], o["K"]) <= R.RTOL and R._rel(cost[i], o["cost_pred"]) <= R.RTOL, (launch, b)
            j = of_parity[b % 2]
            assert R._rel(K[i], Kw[j]) <= R.RTOL and R._rel(cost[i], cw[j]) <= R.RTOL, (launch, b)


def test_wave_pairs_follow_the_count(tiled_base, monkeypatch):
    """batch = #SIMDs / 2 + 2 runs one wave per trajectory; a list of #SIMDs / 2 runs the wave pairs, one more the one-wave forms."""
    c, p, refs = tiled_base
    half = R._n_simd() // 2
    out = _form_run(c, p, half + 2, (half, half + 1), monkeypatch)
    assert ":w1:" in out[0][0][0] and ":w1:" in out[0][0][1], out[0][0]
    assert ":pairh:" in out[1][0][0] and ":pair:" in out[1][0][1] and all(x.endswith(":subset") for x in out[1][0]), out[1][0]
    assert ":w1:" in out[2][0][0] and ":w1:" in out[2][0][1] and all(x.endswith(":subset") for x in out[2][0]), out[2][0]
    _hold(out, refs)


def test_exclusive_twins_follow_the_count(tiled_base, monkeypatch):
    """batch = #SIMDs + 1 runs the plain one-wave kernels; a list of #SIMDs runs their exclusive-SIMD twins, everybody the plain ones.
    kpilqr_last_launch does not name the twin: both are held to the oracle and to the whole-batch sweep."""
    c, p, refs = tiled_base
    n_simd = R._n_simd()
    out = _form_run(c, p, n_simd + 1, (n_simd, n_simd + 1), monkeypatch)
    for (launch, _, _, _) in out:
        assert ":w1:" in launch[0] and ":w1:" in launch[1], launch
    assert all(x.endswith(":subset") for x in out[1][0] + out[2][0])
    _hold(out, refs)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def _raises(code, call, *a, **kw):
    with pytest.raises(KpilqrError) as ei:
        call(*a, **kw)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


@pytest.mark.parametrize("name", ["fused_w1_rxc", "tiled_uw"])
def test_refusals_leave_the_context_as_it_was(name, monkeypatch):
    c = P.ALL_CASES[name][0]
    p0, p1 = P.pair(name)
    lam0 = np.full(P.B, 0.1)
    R._set_env(c, monkeypatch)
    L = _lib.load()
    with R._engine(c, p0) as e:
        if P.is_fused(e):                                   # before any key-points exist
            _raises(ERR_STATE, e.backward_partial, [0, 2])
            _raises(ERR_STATE, e.forward_linear_partial, [0, 2], P.ALPHAS)
            _raises(ERR_STATE, e.iterate_partial, [0, 2], 0.1, 100, P.ALPHAS)
        P.whole(e, c, p0, lam0)
        snap = P.snapshot(e)
        for traj in ([1, 1], [2, 1], [-1, 0], [0, P.B]):    # not increasing, out of range
            _raises(ERR_ARG, e.backward_partial, traj, 0.5)
            _raises(ERR_ARG, e.forward_linear_partial, traj, P.ALPHAS)
            _raises(ERR_ARG, e.iterate_partial, traj, 0.5, 100, P.ALPHAS)
        _raises(ERR_ARG, e.backward_partial, [0, 2], 0.5, 0)                                # pd_check_stride < 1
        _raises(ERR_ARG, e.iterate_partial, [0, 2], 0.5, 0, P.ALPHAS)
        two = np.array([0, 2], np.int32)
        h = e._h
        assert L.kpilqr_backward_partial(h, -1, two.ctypes.data_as(C.c_void_p), None, 100, None, None) == ERR_ARG      # count < 0
        assert L.kpilqr_backward_partial(h, 2, None, None, 100, None, None) == ERR_ARG                                # count > 0, no list
        assert L.kpilqr_forward_linear_partial(h, -1, two.ctypes.data_as(C.c_void_p), None, None, None) == ERR_ARG
        assert L.kpilqr_forward_linear_partial(h, 2, None, None, None, None) == ERR_ARG
        assert L.kpilqr_iterate_partial(h, -1, two.ctypes.data_as(C.c_void_p), None, 100, None) == ERR_ARG
        assert L.kpilqr_iterate_partial(h, 2, None, None, 100, None) == ERR_ARG
        if P.is_fused(e):                                   # ranges pending after kpilqr_update_keypoints
            e.update_keypoints_rows([1], [p0["kp_rows"][1]])
            msg = _raises(ERR_STATE, e.backward_partial, [0, 2], 0.5)
            assert "pending" in msg, msg
            _raises(ERR_STATE, e.forward_linear_partial, [0, 2], P.ALPHAS)
            _raises(ERR_STATE, e.iterate_partial, [0, 2], 0.5, 100, P.ALPHAS)
            xp, xm, md = synth.kp_ordered_payload(p0)
            idx = P.entries_of(p0, [1])
            e.upload_fd_kp_partial([1], e.fd_kp_slab(xp[idx], xm[idx], md[idx]), eps=p0["eps"])
        same = P.snapshot(e)
        for key in snap:                                    # nothing was written
            assert np.array_equal(same[key], snap[key]), key
        e.backward(None)                                    # ... and a whole-batch sweep reproduces the snapshot: lambdas, inputs, state
        e.forward_linear(P.ALPHAS)
        again = P.snapshot(e)
        for key in snap:
            assert np.array_equal(again[key], snap[key]), key


# ---- 7. the batch shim --------------------------------------------------------------------------------------------------------
SHIM_Q0S = np.array([[3.1415, 0.3], [2.6, -0.4], [3.5, 0.1], [1.2, 0.8], [0.4, -1.1], [2.9, 0.9]])


def _shim_pair(method, **kw):
    """iLQR_GPU_Batch on `method` and on `method` + "+activesweeps": the same optimisation, bit for bit, with fewer trajectories swept."""
    from trajoptkp_amd import host
    ref = host.run_acrobot_batch(SHIM_Q0S, method=method, **kw)
    res = host.run_acrobot_batch(SHIM_Q0S, method=method + "+activesweeps", **kw)
    print(f"{method}: iterations {list(ref['iterations'])} lambda_retries {ref['lambda_retries']} backward calls {ref['backward_sweeps']}; "
          f"trajectories swept backward {res['backward_trajectories_swept']} of {ref['backward_trajectories_swept']}, "
          f"forward {res['forward_trajectories_swept']} of {ref['forward_trajectories_swept']}")
    assert np.array_equal(res["cost_history_raw"], ref["cost_history_raw"])
    assert np.array_equal(res["iterations"], ref["iterations"]) and np.array_equal(res["U"], ref["U"])
    assert np.array_equal(res["final_lambda"], ref["final_lambda"])
    assert res["lambda_retries"] == ref["lambda_retries"]
    assert ref["backward_trajectories_swept"] == ref["backward_sweeps"] * len(SHIM_Q0S)
    assert 0 < res["backward_trajectories_swept"] < ref["backward_trajectories_swept"]
    assert 0 < res["forward_trajectories_swept"] < ref["forward_trajectories_swept"]
    return ref, res


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_batched_optimiser_sweeps_the_trajectories_that_need_it(fused):
    """adaptive_accel on the six starts of tests/test_gpu_partial_inputs.py's shim test: trajectories converge at different
    iterations, so the default route sweeps finished ones."""
    ref, _ = _shim_pair("adaptive_accel", T=120, min_N=3, max_iter=9, min_iter=2, torque_weight=1e-3, fused=fused)
    assert len(set(ref["iterations"])) > 1


@pytest.mark.parametrize("devretry", [False, True], ids=["host_retry", "devretry"])
def test_batched_optimiser_retries_the_trajectories_that_failed(devretry):
    """A negative torque weight ("+signedtorque", T = 130: the shims check every 100th step) makes PD checks fail at small lambda,
    as in tests/test_gpu_lambda_retry.py; on the host route each retry sweeps the trajectories that failed, on the device route the
    attempts are listed launches.  "+f32gains" rides along on the device route: the options combine."""
    method = "set_interval+signedtorque" + ("+devretry+f32gains" if devretry else "")
    ref, _ = _shim_pair(method, T=130, min_N=5, max_iter=5, min_iter=2, torque_weight=-0.5, fused=True)
    assert ref["lambda_retries"] > 0
