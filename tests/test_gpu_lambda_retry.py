"""GPU tests of the lambda retry schedule (kpilqr_set_lambda_retry, csrc/lambda_retry.hip and the GATED twins of every backward
kernel): a backward pass whose PD check fails is swept again at lambda * factor on the device, per trajectory, until it settles, the
schedule gives up, or the attempts run out.

Problems, kernel-family cases and the reference loop are those of tests/_lambda_retry.py (batch 4 .. 6, T <= 64; negative running
weights, a PD check every 10 steps, start lambdas 0.1 / 1 / 10 / 1e-4 ... per trajectory), whose attempt counts
tests/test_lambda_retry_model.py asserts on the CPU.  Three references, each made once and shared:
  * the reference loop on the oracle (status, attempts, lambda_used: exact; K, k, delta_J, predicted costs of settled trajectories: the
    suite's 1e-9 relative bar, at lambda_used),
  * the host loop of iLQR_GPU_Batch.cpp:353-373 written here with Engine.backward on a second context without a schedule (bit for bit:
    a settled trajectory's successful sweep is the same launch arithmetic wherever it runs),
  * a context that never saw a schedule (off means off)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import oracle as orc
from trajoptkp_amd import Engine, _lib, synth
from trajoptkp_amd.engine import KpilqrError

import _lambda_retry as lr

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ALPHAS = orc.alphas(6)
ENV_KEYS = ("KPILQR_FUSED_WAVES", "KPILQR_FUSED_FWD_WAVES", "KPILQR_ROLE_SHIFT", "KPILQR_TILED_UW", "KPILQR_TILED_A6")


def same(a, b):
    """bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


def engine(case, upload=True):
    """A context of the case's kernel family (the environment switches are read when it is created), with its problem resident."""
    name, kw, env, kp_ordered, _ = lr.CASES[case]
    p = lr.problem(name)
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        e = Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], **kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    if upload:
        synth.upload(e, p, kp_ordered=kp_ordered)
    return e, p


def staged(e):
    """STEP 1 of a context with records, before kpilqr_backward: A, B of every step, and the cost derivatives unless the tiled sweeps
    form them themselves (the one-tile fused sweeps do all of it)"""
    if "fused" in e.backward_variant:
        return
    e.fd_interpolate()
    if "a6" not in e.backward_variant:
        e.cost_derivs()


def collect(e, with_retry=True):
    K, k = e.gains()
    out = dict(K=K, k=k, launch=e.last_launch("backward"), **e.results())
    if with_retry:
        out["lambda_used"], out["attempts"] = e.lambda_retry()
    return out


def host_loop(e, lam0, factor=lr.FACTOR, max_lambda=lr.MAX_LAMBDA, max_attempts=lr.MAX_ATTEMPTS, forward=False):
    """iLQR_GPU_Batch.cpp:353-373 on a context without a schedule: backward for the whole batch, look at status, raise the lambdas of
    the failed trajectories, again -- until nobody is pending.  -> the final call's outputs, lambda_used, attempts."""
    B = e.batch
    lam = np.array(lam0, np.float64); settled = np.zeros(B, bool); att = np.ones(B, np.int32)
    calls = 0
    while True:
        status, _ = e.backward(lam, pd_stride=lr.PD_STRIDE)
        calls += 1
        again = False
        for b in range(B):
            if settled[b]:
                continue
            nxt = lam[b] * factor
            if status[b] == 0 or nxt > max_lambda or att[b] >= max_attempts:
                settled[b] = True
            else:
                lam[b] = nxt; att[b] += 1; again = True
        if not again:
            break
    if forward:
        e.forward_linear(ALPHAS, fetch=False)
    out = collect(e, with_retry=False)
    out.update(lambda_used=lam, attempts=att, calls=calls)
    return out


@functools.lru_cache(maxsize=None)
def host_reference(case, forward=False):
    e, p = engine(case)
    with e:
        staged(e)
        return host_loop(e, p["lam0"], forward=forward)


def assert_schedule(got, ref, label):
    print(f"{label}: status {list(got['status'])} attempts {list(got['attempts'])} lambda_used {list(got['lambda_used'])}")
    assert list(got["status"]) == list(ref["status"]), (label, got["status"], ref["status"])
    assert list(got["attempts"]) == list(ref["attempts"]), (label, got["attempts"], ref["attempts"])
    assert same(got["lambda_used"], ref["lambda_used"]), (label, got["lambda_used"], ref["lambda_used"])


def assert_oracle(got, ref, label, cost=False):
    for b in np.nonzero(ref["settled"])[0]:
        o = ref["out"][b]
        fig = dict(K=relerr(got["K"][b], o["K"]), k=relerr(got["k"][b], o["k"]), delta_J=abs(got["delta_J"][b] - o["delta_J"]) / abs(o["delta_J"]))
        if cost:
            fig["cost"] = float(np.max(np.abs(got["cost_pred"][b] - o["cost_pred"])) / np.max(np.abs(o["cost_pred"])))
        print(f"{label} b={b} lambda {ref['lambda_used'][b]!r}: " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
        assert all(v < RTOL for v in fig.values()), (label, b, fig)


def assert_same_settled(got, want, settled, label, names=("K", "k", "delta_J", "status")):
    for b in np.nonzero(settled)[0]:
        for name in names:
            assert same(got[name][b], want[name][b]), (label, b, name)


# ---- 1. every family -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(lr.CASES))
def test_every_family_follows_the_schedule(case):
    ref = lr.reference(lr.CASES[case][0])
    e, p = engine(case)
    with e:
        staged(e)
        e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        plain_launch = e.last_launch("backward")                 # the form without a schedule
        e.set_lambda_retry()
        st, dJ = e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        got = collect(e)
    assert lr.CASES[case][4] in got["launch"], got["launch"]
    assert got["launch"] == plain_launch
    assert_schedule(got, ref, case)
    assert list(st) == list(ref["status"]) and same(dJ, got["delta_J"])
    assert_oracle(got, ref, case)
    host = host_reference(case)
    assert list(host["attempts"]) == list(ref["attempts"]) and same(host["lambda_used"], ref["lambda_used"]) and host["calls"] == max(ref["attempts"])
    assert_same_settled(got, host, ref["settled"], case)


# ---- 2. kpilqr_iterate -----------------------------------------------------------------------------------------------------------------
ITERATE_CASES = ("fused_w1_raw", "fused_pair_ragged", "fused_union", "t1_acrobot", "tiled_uw", "tiled_pad8", "wide", "generic")


@pytest.mark.parametrize("case", ITERATE_CASES)
def test_iterate_under_the_schedule(case):
    ref = lr.reference(lr.CASES[case][0])
    e, p = engine(case)
    with e:
        e.set_lambda_retry()
        e.iterate(p["lam0"], lr.PD_STRIDE, ALPHAS)
        got = collect(e)
    assert_schedule(got, ref, case)
    assert_oracle(got, ref, case, cost=True)
    host = host_reference(case, forward=True)
    assert_same_settled(got, host, ref["settled"], case, names=("K", "k", "delta_J", "status", "cost_pred"))


# ---- 3. the streamed calls ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def iterate_reference(case):
    e, p = engine(case)
    with e:
        e.set_lambda_retry()
        e.iterate(p["lam0"], lr.PD_STRIDE, ALPHAS)
        return collect(e)


def stream_setup(e, p, payload):
    e.set_keypoints_rows(p["kp_rows"])
    e.upload_residuals(None, None, None, p["w_run"], p["w_term"])
    e.upload_nominal(None, p["ctrl_lim"])
    e.forward_linear(ALPHAS, fetch=False)
    if payload == "kp_ordered":
        inp = dict(fd_kp=e.fd_kp_slab(*synth.kp_ordered_payload(p)), eps=p["eps"])
    else:
        inp = dict(fd=e.fd_slab(p["job_b"], p["job_t"], p["job_col"], p["job_mode"], p["xplus"], p["xminus"], job_nom=p["job_nom"], xnom=p["xnom"]),
                   eps=p["eps"])
    for name in ("r", "r_x", "r_u", "u_nom"):
        inp[name] = e.pinned(p[name].shape); inp[name][...] = p[name]
    inp["lam"] = e.pinned(p["batch"]); inp["lam"][:] = p["lam0"]
    return inp


def stream_outputs(e, f32):
    B, T, n, m = e.batch, e.T, e.n, e.m
    o = dict(k=e.pinned((B, T, m)), cost_pred=e.pinned((B, e.n_alpha)), delta_J=e.pinned(B), status=e.pinned(B, np.int32))
    o["K32" if f32 else "K"] = e.pinned((B, T, n, m), np.float32 if f32 else np.float64)
    for a in o.values():
        a[...] = -7
    return o


@pytest.mark.parametrize("nchunks", [1, 3])
@pytest.mark.parametrize("case,payload", [("fused_w1_raw", "kp_ordered"), ("fused_pair_shift0", "jobs"), ("t1_acrobot", "kp_ordered"),
                                          ("tiled_pad8", "jobs")])
def test_streamed_iterations_under_the_schedule(case, payload, nchunks):
    """iterate_streamed, then iterate_streamed2 with K32 and a gain list, then two calls with no sync between them: the outputs and
    lambda_retry() of each are those of kpilqr_iterate under the schedule, bit for bit -- every chunk ran its own attempts."""
    want = iterate_reference(case)
    settled = want["status"] == 0
    e, p = engine(case, upload=False)
    with e:
        inp = stream_setup(e, p, payload)
        e.set_lambda_retry()

        def check(o, rows, f32, label):
            lam_used, att = e.lambda_retry()                     # (syncs)
            assert same(lam_used, want["lambda_used"]) and list(att) == list(want["attempts"]), (label, lam_used, att)
            assert same(o["status"], want["status"]), (label, o["status"], want["status"])
            for b in np.nonzero(settled)[0]:
                assert same(o["delta_J"][b], want["delta_J"][b]) and same(o["cost_pred"][b], want["cost_pred"][b]), (label, b)
            for i, b in enumerate(rows):
                if settled[b]:
                    Kw = want["K"][b].astype(np.float32) if f32 else want["K"][b]
                    assert same(o["K32" if f32 else "K"][i], Kw) and same(o["k"][i], want["k"][b]), (label, b)

        B = p["batch"]
        o1 = stream_outputs(e, False)
        e.iterate_streamed(pd_stride=lr.PD_STRIDE, nchunks=nchunks, **inp, **o1)
        check(o1, range(B), False, "streamed")
        rows = [b for b in range(B) if b != 1]
        o2 = stream_outputs(e, True)
        inp["lam"][:] = p["lam0"]
        e.iterate_streamed(pd_stride=lr.PD_STRIDE, nchunks=nchunks, gain_traj=rows, **inp, **o2)
        check(o2, rows, True, "streamed2")
        o3, o4 = stream_outputs(e, False), stream_outputs(e, False)
        lam2 = e.pinned(B); lam2[:] = p["lam0"]
        e.iterate_streamed(pd_stride=lr.PD_STRIDE, nchunks=nchunks, **inp, **o3)
        e.iterate_streamed(pd_stride=lr.PD_STRIDE, nchunks=nchunks, **dict(inp, lam=lam2), **o4)          # no sync in between
        check(o4, range(B), False, "second of two")
        check(o3, range(B), False, "first of two")


# ---- 4. caps and continuation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fused_w1_raw", "tiled_uw"])
def test_caps_continuation_and_another_schedule(case):
    name = lr.CASES[case][0]
    full = lr.reference(name)
    e, p = engine(case)
    with e:
        staged(e)
        # max_attempts = 2: a trajectory that needs three sweeps is out of attempts one multiply up
        e.set_lambda_retry(max_attempts=2)
        st, _ = e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        got = collect(e)
        capped = lr.reference(name, max_attempts=2)
        assert_schedule(got, capped, case + " capped")
        need3 = [b for b in range(p["batch"]) if full["attempts"][b] >= 3 and full["settled"][b]]
        assert need3
        for b in need3:
            assert got["attempts"][b] == 2 and got["status"][b] != 0 and got["lambda_used"][b] == p["lam0"][b] * lr.FACTOR
        # ... and a call with lambda = NULL carries on from the resident lambdas until it settles: the lambdas visited are the reference's
        visited = [[p["lam0"][b], p["lam0"][b] * lr.FACTOR] for b in range(p["batch"])]
        for _ in range(4):
            e.backward(None, pd_stride=lr.PD_STRIDE)
            lam_used, att = e.lambda_retry()
            for b in need3:                               # (the call's first sweep repeats the resident lambda)
                for _ in range(1, att[b]):
                    visited[b].append(visited[b][-1] * lr.FACTOR)
                assert lam_used[b] == visited[b][-1]
            if all(e.results()["status"][b] == 0 for b in need3):
                break
        res = collect(e)
        for b in need3:
            assert res["status"][b] == 0 and tuple(visited[b]) == full["visited"][b], (b, visited[b], full["visited"][b])
        assert_same_settled(res, host_reference(case), np.isin(np.arange(p["batch"]), need3), case + " continued")
        # max_attempts = 1: the unscheduled call
        e.set_lambda_retry(max_attempts=1)
        e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        one = collect(e)
        e.set_lambda_retry(None)
        e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        off = collect(e, with_retry=False)
        assert list(one["attempts"]) == [1] * p["batch"] and same(one["lambda_used"], p["lam0"])
        for nm in ("K", "k", "delta_J", "status"):
            assert same(one[nm], off[nm]), nm
        # another schedule, against the test's own loop on the oracle and on the host
        sched = lr.OTHER_SCHEDULE
        e.set_lambda_retry(**sched)
        e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        got4 = collect(e)
        ref4 = lr.reference(name, **sched)
        assert_schedule(got4, ref4, case + " factor 4")
        assert_oracle(got4, ref4, case + " factor 4")
        e.set_lambda_retry(None)
        assert_same_settled(got4, host_loop(e, p["lam0"], **sched), ref4["settled"], case + " factor 4")


# ---- 5. off means off ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fused_pair_raw", "t1", "tiled_col"])
def test_off_means_off(case):
    """After set_lambda_retry(None) a failing trajectory stays failed after one backward, lambda_retry() is KPILQR_ERR_STATE, and the
    outputs are a fresh context's bit for bit: status of every trajectory, and K, k, delta_J and predicted costs of the SETTLED ones.
    A failed trajectory's gains, delta_J and costs are undefined by the contract of kpilqr_backward -- below its failing step they are
    whatever earlier sweeps left, which on this context were the scheduled call's -- so they are not compared."""
    ref = lr.reference(lr.CASES[case][0], max_attempts=1)
    assert np.any(ref["status"] != 0)
    e, p = engine(case)
    with e:
        staged(e)
        e.backward(p["lam0"], pd_stride=lr.PD_STRIDE); e.forward_linear(ALPHAS, fetch=False)
        fresh = collect(e, with_retry=False)
    e, p = engine(case)
    with e:
        staged(e)
        e.set_lambda_retry()
        e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        e.set_lambda_retry(None)
        with pytest.raises(KpilqrError) as err:
            e.lambda_retry()
        assert err.value.code == _lib.ERR_STATE
        e.backward(p["lam0"], pd_stride=lr.PD_STRIDE); e.forward_linear(ALPHAS, fetch=False)
        off = collect(e, with_retry=False)
        assert list(off["status"]) == list(ref["status"]) and same(off["status"], fresh["status"])      # a failing trajectory stays failed
        assert np.any(ref["settled"])
        assert_same_settled(off, fresh, ref["settled"], case, names=("K", "k", "delta_J", "cost_pred"))       # (the rest is undefined)
        # a schedule set but no sweep under it yet: nothing to download
        e.set_lambda_retry()
        with pytest.raises(KpilqrError) as err:
            e.lambda_retry()
        assert err.value.code == _lib.ERR_STATE


# ---- 6. rejections --------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_context_as_it_was():
    case = "fused_w1_kpc"
    want = host_reference(case)
    ref = lr.reference(lr.CASES[case][0])
    e, p = engine(case)
    L, h = e._L, e._h
    size = C.sizeof(_lib.LambdaRetry)
    bad = [(size - 8, 10.0, 10.0, 6), (size + 8, 10.0, 10.0, 6), (0, 10.0, 10.0, 6),
           (size, 1.0, 10.0, 6), (size, 0.5, 10.0, 6), (size, -10.0, 10.0, 6), (size, float("inf"), 10.0, 6), (size, float("nan"), 10.0, 6),
           (size, 10.0, 0.0, 6), (size, 10.0, -1.0, 6), (size, 10.0, float("inf"), 6), (size, 10.0, float("nan"), 6),
           (size, 10.0, 10.0, 0), (size, 10.0, 10.0, -1), (size, 10.0, 10.0, 65)]
    with e:
        for args in bad:                                 # without a schedule: the context stays without one
            assert L.kpilqr_set_lambda_retry(h, C.byref(_lib.LambdaRetry(*args))) == _lib.ERR_ARG, args
        with pytest.raises(KpilqrError) as err:
            e.lambda_retry()
        assert err.value.code == _lib.ERR_STATE
        e.set_lambda_retry()
        for args in bad:                                 # with one: it stays the one it was
            assert L.kpilqr_set_lambda_retry(h, C.byref(_lib.LambdaRetry(*args))) == _lib.ERR_ARG, args
        assert L.kpilqr_set_lambda_retry(h, C.byref(_lib.LambdaRetry(size, 10.0, 10.0, 64))) == 0      # the ends of the ranges are accepted
        assert L.kpilqr_set_lambda_retry(h, C.byref(_lib.LambdaRetry(size, 10.0, 10.0, 1))) == 0
        e.set_lambda_retry()
        for args in bad[:3] + bad[-1:]:
            assert L.kpilqr_set_lambda_retry(h, C.byref(_lib.LambdaRetry(*args))) == _lib.ERR_ARG, args
        e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        got = collect(e)
        assert_schedule(got, ref, "after rejections")
        assert_same_settled(got, want, ref["settled"], "after rejections")
        # the schedule survives kpilqr_resize; the counts of the old shape do not
        e.resize(p["dof"], p["m"], p["T"])
        with pytest.raises(KpilqrError) as err:
            e.lambda_retry()
        assert err.value.code == _lib.ERR_STATE
        synth.upload(e, p, kp_ordered=False)
        e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        assert_schedule(collect(e), ref, "after resize")


# ---- 7. the host shim ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_host_shim_device_retry_equals_the_host_loop(fused):
    """iLQR_GPU_Batch with "+devretry" against its default route, on acrobot swing-ups whose torque weight is NEGATIVE
    ("+signedtorque", torque_weight = -0.5: the control cost's l_uu = 2 w is negative and Q_uu + lambda I fails its PD check at small
    lambda), so that the default route's own lambda_retries counter is non-zero -- asserted first.  The horizon is 130 steps because the
    shims check every 100th step: at T <= 100 no check ever runs.  Found with the default route on the GPU: torque_weight -0.5, -2 and
    -20 at T = 130 give lambda_retries 15, 15 and 6 (backward_sweeps 9, 9, 3) for these three starts, and 0 at T = 60 whatever the
    weight.  Cost histories, iteration counts, final lambdas and controls are bit-identical between the routes; the device route calls
    kpilqr_backward once per iteration."""
    from trajoptkp_amd import host
    q0s = np.array([[3.1415, 0.3], [2.9, -0.2], [3.3, 0.1]])
    kw = dict(T=130, min_N=5, max_iter=4, min_iter=2, torque_weight=-0.5, fused=fused)
    a = host.run_acrobot_batch(q0s, method="set_interval+signedtorque", **kw)
    print("default route: backward_sweeps", a["backward_sweeps"], "lambda_retries", a["lambda_retries"], "final lambda", a["final_lambda"])
    assert a["lambda_retries"] > 0
    b = host.run_acrobot_batch(q0s, method="set_interval+signedtorque+devretry", **kw)
    print("device route:  backward_sweeps", b["backward_sweeps"], "lambda_retries", b["lambda_retries"], "final lambda", b["final_lambda"])
    assert same(a["cost_history_raw"], b["cost_history_raw"])
    assert list(a["iterations"]) == list(b["iterations"])
    assert same(a["final_lambda"], b["final_lambda"])
    assert same(a["U"], b["U"])
    assert a["lambda_retries"] == b["lambda_retries"]
    assert b["backward_sweeps"] < a["backward_sweeps"]
