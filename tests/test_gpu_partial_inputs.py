"""GPU tests of the second half of partial re-linearisation: kpilqr_upload_residuals_partial / kpilqr_upload_nominal_partial send the
rows of SOME trajectories, kpilqr_fd_interpolate_partial / kpilqr_cost_derivs_partial rewrite the step records of those trajectories
alone (the kernels of elementwise.hip / linearise.hip take the trajectory of a block row from a device list).

Two problems p0 and p1 of one shape with different seeds; "merged" is p1 for the listed trajectories and p0 elsewhere.  The yardstick
of every result is a FRESH context that is given the merged arrays through the whole-batch calls, and every comparison is
np.array_equal: the partial calls copy bytes and run the same arithmetic on the same inputs.  T = 53 leaves a ragged last block for
every kernel here (the 16-step interpolation tile, the 12 / 9 / 51-step tiles of k_cost_derivs_rows<14,7> / <20,7> / <4,1>, the
4-step tile of k_cost_derivs); B = 6."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from trajoptkp_amd import Engine, _lib, host, synth
from trajoptkp_amd.engine import KpilqrError, rows_to_dof_csr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -5
ALPHAS = orc.alphas(6)
T, B = 53, 6
SUBSETS = {"first": [0], "last": [B - 1], "run": [1, 2, 3], "gaps": [0, 2, 5], "all": list(range(B)), "none": []}
SUBSET_IDS = list(SUBSETS)
PER_TRAJ = ("r", "r_x", "r_u", "u_nom")


# ---- problems -----------------------------------------------------------------------------------------------------------------
def _rows(task, seed):
    dof = synth._task_cfg(task)[1]["dof"]
    rng = np.random.default_rng(seed)
    return synth.bisect_keypoints(rng, dof, T, 1, rng.uniform(0.2, 1.0, dof))


def _problem(task, rows, config_id):
    """Per-DoF lists, a fraction of one-sided jobs, dense r_x and r_u; a trajectory's data depend on (config_id, its index, its lists)
    alone."""
    p = synth.make_ragged_problem(task, T, list(rows), config_id=config_id, one_sided_frac=0.3)
    keep = p["job_col"] < p["n"] + min(p["m"], p["dof"])      # (control columns without a DoF list have no slot in a by-entry payload)
    for k in ("job_b", "job_t", "job_col", "job_mode", "job_nom", "xplus", "xminus"):
        p[k] = p[k][keep]
    return p


@functools.lru_cache(maxsize=None)
def _pair(task, new_lists):
    """(p0, p1): new_lists = False: the same key-point lists in both (only the per-iteration inputs differ)."""
    rows0 = [_rows(task, 100 * b + T) for b in range(B)]
    rows1 = [_rows(task, 7000 + b) for b in range(B)] if new_lists else rows0
    return _problem(task, rows0, 31), _problem(task, rows1, 32)


def _merged(p0, p1, who):
    """p1 for the trajectories of `who`, p0 elsewhere: lists, FD jobs (sorted by trajectory), residuals, nominal controls."""
    q = dict(p0)
    sel = np.zeros(B, bool); sel[list(who)] = True
    q["kp_rows"] = [p1["kp_rows"][b] if sel[b] else p0["kp_rows"][b] for b in range(B)]
    for k in PER_TRAJ:
        q[k] = np.where(sel.reshape((B,) + (1,) * (p0[k].ndim - 1)), p1[k], p0[k])
    k0, k1 = ~sel[p0["job_b"]], sel[p1["job_b"]]
    jobs = {k: np.concatenate([p0[k][k0], p1[k][k1]]) for k in ("job_b", "job_t", "job_col", "job_mode", "xplus", "xminus")}
    jobs["job_nom"] = np.concatenate([p0["job_nom"][k0], p1["job_nom"][k1] + len(p0["xnom"])])
    order = np.argsort(jobs["job_b"], kind="stable")
    for k, v in jobs.items():
        q[k] = v[order]
    q["xnom"] = np.concatenate([p0["xnom"], p1["xnom"]])
    return q


def _engine(p, monkeypatch=None, env=None, **kw):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    e = Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)                 # read once, in kpilqr_create
    assert ("fused" in e.backward_variant) == bool(kw.get("fused"))
    return e


def _entries_of(p, traj):
    o, _ = rows_to_dof_csr(p["kp_rows"], p["dof"], p["T"])
    dof = p["dof"]
    return np.concatenate([np.arange(o[b * dof], o[(b + 1) * dof]) for b in traj]) if len(traj) else np.zeros(0, np.int64)


def _payload(e, p, form, traj=None):
    """The whole payload of p, or (traj) that of those trajectories alone: their entries back to back through the partial call, or
    -- job lists carry their own indices -- their jobs."""
    if form == "jobs":
        s = np.ones(len(p["job_b"]), bool) if traj is None else np.isin(p["job_b"], traj)
        e.upload_fd(p["job_b"][s], p["job_t"][s], p["job_col"][s], p["job_mode"][s], p["xplus"][s], p["xminus"][s], job_nom=p["job_nom"][s],
                    xnom=p["xnom"], eps=p["eps"])
        return
    xp, xm, md = synth.kp_ordered_payload(p)
    if traj is not None:
        idx = _entries_of(p, traj)
        xp, xm, md = xp[idx], xm[idx], md[idx]
    if form == "fd_kp":
        s = e.fd_kp_slab(xp, xm, md)
        e.upload_fd_kp(s, eps=p["eps"]) if traj is None else e.upload_fd_kp_partial(traj, s, eps=p["eps"])
    else:
        s = e.kp_columns(xp, xm, md, eps=p["eps"])
        e.upload_kp_columns(s) if traj is None else e.upload_kp_columns_partial(traj, s)


def _rest(e, p):
    e.upload_residuals(p["r"], p["r_x"], p["r_u"], p["w_run"], p["w_term"])
    e.upload_nominal(p["u_nom"], p["ctrl_lim"])


def _rest_partial(e, p, who):
    e.upload_residuals_partial(who, p["r"][who], p["r_x"][who], p["r_u"][who])
    e.upload_nominal_partial(who, p["u_nom"][who])


def _buffers(e, p, which=("r", "r_x", "r_u", "u_nom")):
    ids = dict(r=_lib.BUF_RESIDUALS, r_x=_lib.BUF_R_X, r_u=_lib.BUF_R_U, u_nom=_lib.BUF_U_NOM)
    e.sync()
    return {k: e._d2h(ids[k], p[k].shape, np.float64) for k in which}


def _iterate(e, p):
    e.iterate(p["lam"], 100, ALPHAS)
    res = e.results()
    K, k = e.gains()
    return dict(K=K, k=k, delta_J=res["delta_J"], cost=res["cost_pred"], status=res["status"],
                launch=np.array([e.last_launch("backward"), e.last_launch("forward")]))


def _same(got, want, what):
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), (what, key)


def _raises(code, call, *a, **kw):
    with pytest.raises(KpilqrError) as ei:
        call(*a, **kw)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


# ---- 1. rows of a subset ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", SUBSET_IDS)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
@pytest.mark.parametrize("task", ["acrobot", "panda_reaching"])          # (acrobot: nr = 5, odd)
def test_rows_of_a_subset_land_in_place(task, fused, subset):
    p0, p1 = _pair(task, False)
    who = SUBSETS[subset]
    pm = _merged(p0, p1, who)
    with _engine(p0, fused=fused) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, "fd_kp")
        _rest(e, p0)
        _rest_partial(e, p1, who)
        got = _iterate(e, pm)
        buf = _buffers(e, pm)          # (behind the iteration: a writable r_x / r_u pointer leaving the library changes the context's state)
    for k in PER_TRAJ:
        assert np.array_equal(buf[k], pm[k]), k
    with _engine(p0, fused=fused) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, "fd_kp")
        _rest(e, pm)
        want = _iterate(e, pm)
    assert np.all(want["status"] == 0) and np.any(want["K"] != 0)
    _same(got, want, (task, fused, subset))
    if who:
        assert not np.array_equal(pm["r"], p0["r"])


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------
def test_jacobian_rows_are_refused_where_they_would_change_the_form_of_the_sweeps(monkeypatch):
    p0, p1 = _pair("panda_reaching", False)
    who = [1, 4]
    rows = lambda k: p1[k][who]
    rxc = np.zeros((p0["nr"], p0["n"])); rxc[np.arange(p0["nr"]), np.arange(p0["nr"]) % p0["n"]] = 1.0
    one_wave = {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}

    def run(refused):
        """Constant-Jacobian mode and no control residuals; `refused`: the calls that must change nothing come first."""
        with _engine(p0, monkeypatch, one_wave, fused=True) as e:
            e.set_keypoints_rows(p0["kp_rows"])
            _payload(e, p0, "fd_kp")
            e.upload_residuals(p0["r"], None, None, p0["w_run"], p0["w_term"])
            e.upload_residual_jacobians_const(rxc)
            e.upload_nominal(p0["u_nom"], p0["ctrl_lim"])
            if refused:
                msg = _raises(ERR_STATE, e.upload_residuals_partial, who, rows("r"), rows("r_x"))        # r_x in constant-Jacobian mode
                assert "kpilqr_upload_residuals" in msg and "constant" in msg, msg
                msg = _raises(ERR_STATE, e.upload_residuals_partial, who, rows("r"), None, rows("r_u"))  # r_u on a context that never had one
                assert "kpilqr_upload_residuals" in msg and "r_u" in msg, msg
                assert np.array_equal(_buffers(e, p0, ("r",))["r"], p0["r"])                              # the r of the same calls did not go either
            out = _iterate(e, p0)
            assert ":ru0" in out["launch"][0] and ":rxc" in out["launch"][0], out["launch"]      # neither mode was flipped
            if refused:                       # (read last: these pointers end the modes)
                buf = _buffers(e, p0, ("r_u",))
                assert not np.any(buf["r_u"])
        return out
    _same(run(True), run(False), "refused calls change nothing")
    # r_x before any whole r_x: the buffer's other rows mean nothing yet
    with _engine(p0) as e:
        _raises(ERR_STATE, e.upload_residuals_partial, who, rows("r"), rows("r_x"))
        buf = _buffers(e, p0, ("r", "r_x"))
        assert not np.any(buf["r"]) and not np.any(buf["r_x"])
        e.upload_residuals_partial(who, rows("r"))                                                   # r has no precondition
        e.upload_residuals(None, p0["r_x"], None)
        e.upload_residuals_partial(who, None, rows("r_x"))                                           # ... and r_x none behind a whole one
        buf = _buffers(e, p0, ("r", "r_x"))
        assert np.array_equal(buf["r"][who], rows("r")) and not np.any(np.delete(buf["r"], who, 0))
        assert np.array_equal(buf["r_x"][who], rows("r_x")) and np.array_equal(np.delete(buf["r_x"], who, 0), np.delete(p0["r_x"], who, 0))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_bad_lists_are_refused_by_every_call(fused):
    p0, p1 = _pair("acrobot", False)
    with _engine(p0, fused=fused) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, "fd_kp")
        _rest(e, p0)
        two = lambda k: p1[k][[0, 1]]
        for traj in ([1, 1], [2, 1], [-1, 0], [0, B]):                                       # unsorted, repeated, out of range
            _raises(ERR_ARG, e.upload_residuals_partial, traj, two("r"), two("r_x"), two("r_u"))
            _raises(ERR_ARG, e.upload_nominal_partial, traj, two("u_nom"))
            _raises(ERR_ARG, e.fd_interpolate_partial, traj)
            _raises(ERR_ARG, e.cost_derivs_partial, traj)
        if fused:                             # no persistent records: both record calls are refused, whatever the list
            for call in (e.fd_interpolate_partial, e.cost_derivs_partial):
                assert "KPILQR_FLAG_FUSED" in _raises(ERR_STATE, call, [0, 2])
        buf = _buffers(e, p0)
        for k in PER_TRAJ:
            assert np.array_equal(buf[k], p0[k]), k


def test_fd_interpolate_partial_obeys_the_payload_state():
    p0, p1 = _pair("panda_reaching", True)
    who = [1, 2]
    pm = _merged(p0, p1, who)
    with _engine(p0) as e:
        _raises(ERR_STATE, e.fd_interpolate_partial, who)                                    # before key-points exist
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, "fd_kp")
        e.fd_interpolate()
        fill = _sentinel(p0)
        e.set_AB(*fill)
        e.update_keypoints_rows(who, [p1["kp_rows"][b] for b in who])
        msg = _raises(ERR_STATE, e.fd_interpolate_partial, who)                              # ranges pending
        assert "pending" in msg and "partial" in msg, msg
        assert e.last_launch("linearise") == "fd_kp_interpolate"
        _payload(e, pm, "fd_kp", who)
        A, Bm = e.get_AB()
        assert np.array_equal(A, fill[0]) and np.array_equal(Bm, fill[1])                    # the refused calls wrote nothing
        e.fd_interpolate_partial(who)
        assert e.last_launch("linearise") == "fd_kp_interpolate:subset"


# ---- 3. linearisation of a subset ---------------------------------------------------------------------------------------------
def _sentinel(p):
    n, m = p["n"], p["m"]
    A = 1000.0 + np.arange(B * T * n * n, dtype=np.float64).reshape(B, T, n, n)
    Bm = -1000.0 - np.arange(B * T * m * n, dtype=np.float64).reshape(B, T, m, n)
    return A, Bm


@functools.lru_cache(maxsize=None)
def _oracle_AB(task, b, which):
    """a2 + a4 of the oracle for trajectory b of p0 (which = 0) or p1 (1), on records that start zeroed."""
    p = _pair(task, True)[which]
    n, m, dof = p["n"], p["m"], p["dof"]
    A = np.zeros((T, n, n)); Bm = np.zeros((T, m, n))
    sel = p["job_b"] == b
    orc.fd_difference(n, m, p["job_t"][sel], p["job_col"][sel], p["job_mode"][sel], p["job_nom"][sel], p["xplus"][sel], p["xminus"][sel],
                      p["xnom"], p["eps"], A, Bm)
    offs, cols = p["kp_rows"][b]
    orc.interpolate(dof, m, T, offs, cols, A, Bm)
    return A, Bm


@functools.lru_cache(maxsize=None)
def _fresh_AB(task, form, subset, interp_env):
    """A fresh context: merged lists and payload, the whole-batch call."""
    import os
    p0, p1 = _pair(task, True)
    pm = _merged(p0, p1, SUBSETS[subset])
    old = os.environ.get("KPILQR_FD_INTERP")
    if interp_env is not None:
        os.environ["KPILQR_FD_INTERP"] = interp_env
    try:
        e = _engine(pm)
    finally:
        os.environ.pop("KPILQR_FD_INTERP", None)
        if old is not None:
            os.environ["KPILQR_FD_INTERP"] = old
    with e:
        e.set_keypoints_rows(pm["kp_rows"])
        _payload(e, pm, form)
        e.fd_interpolate()
        return e.get_AB() + (e.last_launch("linearise"),)


LIN_CASES = [("panda_reaching", "fd_kp"), ("panda_pushing", "fd_kp"), ("high_dof_push", "fd_kp"), ("acrobot", "fd_kp"), ("acrobot", "cols"),
             ("acrobot", "jobs")]


@pytest.mark.parametrize("interp_env", [None, "0"], ids=["one_pass", "FD_INTERP=0"])
@pytest.mark.parametrize("subset", SUBSET_IDS)
@pytest.mark.parametrize("task,form", LIN_CASES, ids=[f"{t}-{f}" for t, f in LIN_CASES])
def test_linearisation_of_a_subset(task, form, subset, interp_env, monkeypatch):
    p0, p1 = _pair(task, True)
    who = SUBSETS[subset]
    pm = _merged(p0, p1, who)
    fill = _sentinel(p0)
    env = {} if interp_env is None else {"KPILQR_FD_INTERP": interp_env}
    with _engine(p0, monkeypatch, env) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, form)
        e.fd_interpolate()
        whole = e.last_launch("linearise")
        e.set_AB(*fill)
        e.update_keypoints_rows(who, [p1["kp_rows"][b] for b in who])
        if who or form != "jobs":
            _payload(e, pm, form, who)
        e.fd_interpolate_partial(who)
        how = e.last_launch("linearise")
        A, Bm = e.get_AB()
    wA, wB, whow = _fresh_AB(task, form, subset, interp_env)
    sequence = form == "jobs" or interp_env == "0"
    assert whole == whow == ("fd_difference+interpolate" if sequence else "kp_columns_interpolate" if form == "cols" else "fd_kp_interpolate")
    assert how == (whole + ":subset" if who else whole)          # (nobody listed: a no-op, the whole-batch call's string stays)
    rest = [b for b in range(B) if b not in who]
    assert np.array_equal(A[who], wA[who]) and np.array_equal(Bm[who], wB[who])
    assert np.array_equal(A[rest], fill[0][rest]) and np.array_equal(Bm[rest], fill[1][rest])      # the sentinel, in every element
    for b in who:
        oA, oB = _oracle_AB(task, b, 1)
        assert np.array_equal(A[b], oA) and np.array_equal(Bm[b], oB), b
    if who:
        assert np.any(wA[who] != 0) and np.any(wB[who] != 0)


# ---- 4. cost derivatives of a subset ------------------------------------------------------------------------------------------
def _cost_sentinel(p):
    n, m = p["n"], p["m"]
    rng = np.random.default_rng(5)
    l_xx = rng.standard_normal((B, T, n, n)); l_uu = rng.standard_normal((B, T, m, m))
    return (100.0 + rng.standard_normal((B, T, n)), 200.0 + l_xx + l_xx.transpose(0, 1, 3, 2), 300.0 + rng.standard_normal((B, T, m)),
            400.0 + l_uu + l_uu.transpose(0, 1, 3, 2))


@functools.lru_cache(maxsize=None)
def _fresh_cost(task, subset):
    p0, p1 = _pair(task, False)
    pm = _merged(p0, p1, SUBSETS[subset])
    with _engine(pm) as e:
        e.upload_residuals(pm["r"], pm["r_x"], pm["r_u"], pm["w_run"], pm["w_term"])
        e.cost_derivs()
        return e.get_cost_derivs()


@pytest.mark.parametrize("subset", SUBSET_IDS)
@pytest.mark.parametrize("task", ["acrobot", "panda_reaching", "panda_pushing", "hopper", "high_dof_push"])      # hopper, n = 62: k_cost_derivs
def test_cost_derivatives_of_a_subset(task, subset):
    p0, p1 = _pair(task, False)
    who = SUBSETS[subset]
    fill = _cost_sentinel(p0)
    with _engine(p0) as e:
        e.upload_residuals(p0["r"], p0["r_x"], p0["r_u"], p0["w_run"], p0["w_term"])
        e.cost_derivs()
        first = e.get_cost_derivs()
        e.set_cost_derivs(*fill)
        e.upload_residuals_partial(who, p1["r"][who], p1["r_x"][who], p1["r_u"][who])
        e.cost_derivs_partial(who)
        got = e.get_cost_derivs()
    want = _fresh_cost(task, subset)
    rest = [b for b in range(B) if b not in who]
    for g, w, f, f0 in zip(got, want, fill, first):
        assert np.array_equal(g[who], w[who]) and np.array_equal(g[rest], f[rest])
        assert np.any(f0 != 0) and (not who or not np.array_equal(w[who], f0[who]))


@pytest.mark.parametrize("task", ["panda_reaching", "hopper"])
def test_cost_derivatives_in_constant_jacobian_mode(task):
    """Everybody listed: the call makes the broadcast copy of the constant Jacobians exactly as kpilqr_cost_derivs does."""
    p0, _ = _pair(task, False)
    rxc = np.random.default_rng(3).standard_normal((p0["nr"], p0["n"]))
    out = []
    for partial in (False, True):
        with _engine(p0) as e:
            e.upload_residuals(p0["r"], None, None, p0["w_run"], p0["w_term"])
            e.upload_residual_jacobians_const(rxc)
            e.set_cost_derivs(*_cost_sentinel(p0))
            e.cost_derivs_partial(list(range(B))) if partial else e.cost_derivs()
            out.append(e.get_cost_derivs())
    assert np.any(out[0][1] != 0)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- 5. end to end on records -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", ["gaps", "run"])
def test_partial_linearisation_end_to_end_on_records(subset):
    task = "panda_pushing"
    p0, p1 = _pair(task, True)
    who = SUBSETS[subset]
    pm = _merged(p0, p1, who)
    with _engine(p0) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, "fd_kp")
        _rest(e, p0)
        first = _iterate(e, p0)
        e.update_keypoints_rows(who, [p1["kp_rows"][b] for b in who])
        _payload(e, pm, "fd_kp", who)
        _rest_partial(e, pm, who)
        e.fd_interpolate_partial(who)
        e.cost_derivs_partial(who)
        status, dJ = e.backward(pm["lam"])
        cost = e.forward_linear(ALPHAS)
        K, k = e.gains()
        got = dict(K=K, k=k, delta_J=dJ, cost=cost, status=status, launch=np.array([e.last_launch("backward"), e.last_launch("forward")]),
                   variant=np.array(e.backward_variant))
    with _engine(pm) as e:
        e.set_keypoints_rows(pm["kp_rows"])
        _payload(e, pm, "fd_kp")
        _rest(e, pm)
        want = _iterate(e, pm)
        want["variant"] = np.array(e.backward_variant)
    assert np.all(want["status"] == 0) and not np.array_equal(want["K"], first["K"])
    _same(got, want, subset)


def test_a_whole_linearisation_behind_the_per_run_launches_of_a_subset(monkeypatch):
    """KPILQR_FD_INTERP=0 on the records context above: kpilqr_fd_interpolate_partial scatters the columns of the `gaps` subset with
    one k_kpc_to_records launch per run of adjacent trajectories, each over that run's entry range.  The ranges are arguments of the
    launch: the context's own range is still the whole payload afterwards, so a whole-batch kpilqr_fd_interpolate behind the subset
    call rewrites EVERY record (they are overwritten with a sentinel in between: key-point columns it skipped would stay the
    sentinel's, and k_interpolate would spread them) -- bit for bit what a fresh context makes of the merged problem."""
    task = "panda_pushing"
    p0, p1 = _pair(task, True)
    who = SUBSETS["gaps"]
    pm = _merged(p0, p1, who)
    with _engine(p0, monkeypatch, {"KPILQR_FD_INTERP": "0"}) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, "fd_kp")
        e.fd_interpolate()
        e.update_keypoints_rows(who, [p1["kp_rows"][b] for b in who])
        _payload(e, pm, "fd_kp", who)
        e.fd_interpolate_partial(who)
        assert e.last_launch("linearise") == "fd_difference+interpolate:subset"
        e.set_AB(*_sentinel(p0))
        e.fd_interpolate()
        assert e.last_launch("linearise") == "fd_difference+interpolate"
        A, Bm = e.get_AB()
    wA, wB, whow = _fresh_AB(task, "fd_kp", "gaps", "0")
    assert whow == "fd_difference+interpolate" and np.any(wA != 0) and np.any(wB != 0)
    assert np.array_equal(A, wA) and np.array_equal(Bm, wB)


# ---- 6. the batch shim --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constjac", [False, True], ids=["jacobians", "constjac"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_batched_optimiser_sends_the_inputs_of_the_regenerating_trajectories_alone(fused, constjac):
    """adaptive_accel on the six starts of tests/test_gpu_partial_regeneration.py's shim test: trajectories have steps rejected and
    converge at different iterations.  "+wholeinputs" is the shim as it was: whole-batch residuals at every linearisation, whole-batch
    nominal controls at every iteration, whole-batch record passes."""
    q0s = np.array([[3.1415, 0.3], [2.6, -0.4], [3.5, 0.1], [1.2, 0.8], [0.4, -1.1], [2.9, 0.9]])
    Th, n, m, nr = 120, 4, 1, 5
    method = "adaptive_accel" + ("+constjac" if constjac else "")
    kw = dict(T=Th, min_N=3, max_iter=9, min_iter=2, torque_weight=1e-3, fused=fused)
    res = host.run_acrobot_batch(q0s, method=method, **kw)
    ref = host.run_acrobot_batch(q0s, method=method + "+wholeinputs", **kw)
    assert np.array_equal(res["iterations"], ref["iterations"]) and np.array_equal(res["U"], ref["U"])
    assert len(res["cost_history"]) == len(ref["cost_history"]) and all(np.array_equal(a, b) for a, b in zip(res["cost_history"], ref["cost_history"]))
    assert np.array_equal(res["keypoint_entries"], ref["keypoint_entries"])
    whole_r = len(ref["keypoint_entries"]) * len(q0s) * (Th + 1) * nr * (1 if constjac else 1 + n + m) * 8
    whole_u = int(ref["iterations"].max()) * len(q0s) * Th * m * 8
    print(f"residuals up {res['residual_bytes_uploaded']} of {whole_r} bytes, nominal controls up {res['nominal_bytes_uploaded']} of {whole_u} bytes")
    assert len(ref["keypoint_entries"]) >= 2
    assert ref["residual_bytes_uploaded"] == whole_r and ref["nominal_bytes_uploaded"] == whole_u
    assert 0 < res["residual_bytes_uploaded"] < whole_r
    assert 0 < res["nominal_bytes_uploaded"] < whole_u
