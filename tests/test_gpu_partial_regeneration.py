"""GPU tests of partial re-linearisation: kpilqr_update_keypoints gives SOME trajectories new key-point lists and keeps the resident
payload of the others (their records are moved on the device, csrc/kp_partial.hip), kpilqr_upload_fd_kp_partial /
kpilqr_upload_kp_columns_partial fill in the listed trajectories' ranges, kpilqr_download_gains_partial brings back the gains of a
subset.

The yardstick of every result is a FRESH context that is given the merged lists with set_keypoints and the full payload.  Every
comparison is np.array_equal: the relocation copies bytes, so the sweeps must see identical inputs."""
import functools

import numpy as np
import pytest

from _sequences import _entries_of
from oracle import oracle as orc
from trajoptkp_amd import Engine, host, synth
from trajoptkp_amd.engine import KpilqrError, rows_to_dof_csr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -5
ALPHAS = orc.alphas(6)
TASKS = {"acrobot": (33, 6), "panda_reaching": (40, 4), "panda_pushing": (50, 3)}        # task -> (T, B)
# context -> (Engine keywords, environment read by kpilqr_create, payload form)
CONTEXTS = {
    "fused": (dict(fused=True), {}, "fd_kp"),
    "fused_w1": (dict(fused=True), {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}, "fd_kp"),
    "fused_noraw": (dict(fused=True), {"KPILQR_FUSED_RAW": "0"}, "fd_kp"),
    "records": (dict(), {}, "fd_kp"),                      # materialising: one tile (acrobot, Panda reaching) or tiled (panda_pushing)
    "fused_cols": (dict(fused=True), {}, "cols"),
    "records_cols": (dict(), {}, "cols"),
}
CASES = [(task, ctx) for task in ("acrobot", "panda_reaching") for ctx in CONTEXTS] + [("panda_pushing", "records"), ("panda_pushing", "records_cols")]


# ---- problems -----------------------------------------------------------------------------------------------------------------
def _dof(task):
    return synth._task_cfg(task)[1]["dof"]


def _bisected(task, T, seed):
    dof = _dof(task)
    rng = np.random.default_rng(seed)
    return synth.bisect_keypoints(rng, dof, T, 1, rng.uniform(0.2, 1.0, dof))


def _minimal(task, T):
    return synth.rows_from_dof_lists(_dof(task), T, [[0, T - 1]] * _dof(task))


def _every_step(task, T):
    return synth.rows_from_dof_lists(_dof(task), T, [list(range(T))] * _dof(task))


def _problem(task, T, rows):
    """Per-DoF lists, a fraction of one-sided records; a trajectory's FD data depend on its own lists and its index alone, so a
    trajectory that keeps its lists has the same records in the problem before and after an update."""
    p = synth.make_ragged_problem(task, T, list(rows), config_id=11, one_sided_frac=0.3)
    keep = p["job_col"] < p["n"] + min(p["m"], p["dof"])      # (control columns without a DoF list have no slot in a by-entry payload)
    for k in ("job_b", "job_t", "job_col", "job_mode", "job_nom", "xplus", "xminus"):
        p[k] = p[k][keep]
    return p


@functools.lru_cache(maxsize=None)
def _base(task):
    T, B = TASKS[task]
    return _problem(task, T, [_bisected(task, T, 100 * b + T) for b in range(B)])


def _subsets(task):
    """name -> {trajectory: new rows}: the first, the last, an interior pair whose first shrinks to the minimal list while a later one
    grows to every step (kept ranges move both ways), everybody, nobody."""
    T, B = TASKS[task]
    other = lambda b: _bisected(task, T, 7000 + b)
    return {
        "first": {0: other(0)},
        "last": {B - 1: other(B - 1)},
        "pair": {1: _minimal(task, T), B - 2 if B > 3 else 2: _every_step(task, T)},
        "all": {b: other(b) for b in range(B)},
        "none": {},
    }


def _merged(p, new_rows):
    rows = list(p["kp_rows"])
    for b, r in new_rows.items():
        rows[b] = r
    return _problem(p["task"], p["T"], rows)


# ---- contexts -----------------------------------------------------------------------------------------------------------------
def _engine(p, ctx, monkeypatch):
    kw, env, _ = CONTEXTS[ctx]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], **kw)
    for k in env:
        monkeypatch.delenv(k)                 # read once, in kpilqr_create
    assert ("fused" in e.backward_variant) == bool(kw.get("fused"))
    return e


def _payload(e, p, form, traj=None, eps=None, full_call=False):
    """The whole payload of p, or (traj) the records of those trajectories back to back through the partial call."""
    xp, xm, md = synth.kp_ordered_payload(p)
    if traj is not None and not full_call:
        idx = _entries_of(p, traj)
        xp, xm, md = xp[idx], xm[idx], md[idx]
    eps = p["eps"] if eps is None else eps
    if form == "fd_kp":
        s = e.fd_kp_slab(xp, xm, md)
        e.upload_fd_kp(s, eps=eps) if traj is None or full_call else e.upload_fd_kp_partial(traj, s, eps=eps)
    else:
        s = e.kp_columns(xp, xm, md, eps=p["eps"])
        e.upload_kp_columns(s) if traj is None or full_call else e.upload_kp_columns_partial(traj, s)


def _rest(e, p):
    e.upload_residuals(p["r"], p["r_x"], p["r_u"] if np.any(p["r_u"]) else None, p["w_run"], p["w_term"])
    e.upload_nominal(p["u_nom"], p["ctrl_lim"])


def _iterate(e, p, ctx):
    e.iterate(p["lam"], 100, ALPHAS)
    res = e.results()
    K, k = e.gains()
    out = dict(K=K, k=k, delta_J=res["delta_J"], cost=res["cost_pred"], status=res["status"])
    if "records" in ctx:                      # (a fused context holds no records)
        out["A"], out["B"] = e.get_AB()
    return out


def _yardstick(p, ctx, monkeypatch):
    with _engine(p, ctx, monkeypatch) as e:
        e.set_keypoints_rows(p["kp_rows"])
        _payload(e, p, CONTEXTS[ctx][2])
        _rest(e, p)
        out = _iterate(e, p, ctx)
    assert np.all(out["status"] == 0) and np.any(out["K"] != 0)
    return out


def _update(e, p_new, new_rows, form, rest=True):
    traj = sorted(new_rows)
    e.update_keypoints_rows(traj, [new_rows[b] for b in traj])
    _payload(e, p_new, form, traj)
    if rest:
        _rest(e, p_new)


def _same(got, want, what):
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), (what, key)


# ---- 1. bit-identical results after a partial update --------------------------------------------------------------------------
@pytest.mark.parametrize("subset", ["first", "last", "pair", "all", "none"])
@pytest.mark.parametrize("task,ctx", CASES, ids=[f"{t}-{c}" for t, c in CASES])
def test_partial_update_gives_the_results_of_a_fresh_context(task, ctx, subset, monkeypatch):
    p0 = _base(task)
    new_rows = _subsets(task)[subset]
    p1 = _merged(p0, new_rows)
    form = CONTEXTS[ctx][2]
    with _engine(p0, ctx, monkeypatch) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, form)
        _rest(e, p0)
        first = _iterate(e, p0, ctx)
        # count = 0 must leave everything alone, the validity of the column store included: nothing else is sent either
        _update(e, p1, new_rows, form, rest=subset != "none")
        got = _iterate(e, p1, ctx)
        launch = e.last_launch("backward")
        o, t = e.get_keypoints()
    want = _yardstick(p1, ctx, monkeypatch)
    _same(got, want, (task, ctx, subset))
    wo, wt = rows_to_dof_csr(p1["kp_rows"], p1["dof"], p1["T"])
    assert np.array_equal(o, wo) and np.array_equal(t, wt)
    if subset == "none":
        _same(got, first, "unchanged")
        if ctx == "fused_noraw":              # the column store stayed valid: the second backward sweep read it, no differencing ran
            assert ":kpc:" in launch + ":", launch
    else:
        assert not np.array_equal(got["K"], first["K"])


# ---- 2. growth past the capacity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,ctx", [("panda_reaching", "fused"), ("panda_reaching", "fused_cols"), ("acrobot", "records"), ("panda_pushing", "records")])
def test_growth_beyond_the_capacity_keeps_the_kept_records(task, ctx, monkeypatch):
    """Every trajectory starts on the minimal lists; one grows to every step, which exceeds the payload buffers' capacity (their
    slack is a quarter plus 4 KB: the test checks that its sizes are beyond it)."""
    T, B = TASKS[task]
    p0 = _problem(task, T, [_minimal(task, T)] * B)
    new_rows = {1: _every_step(task, T)}
    p1 = _merged(p0, new_rows)
    e0 = rows_to_dof_csr(p0["kp_rows"], p0["dof"], T)[0][-1]
    e1 = rows_to_dof_csr(p1["kp_rows"], p1["dof"], T)[0][-1]
    rec = (6 * p0["n"] + 2) * 8 if CONTEXTS[ctx][2] == "fd_kp" else 3 * p0["n"] * 8
    assert e1 * rec > e0 * rec + e0 * rec // 4 + 4096
    form = CONTEXTS[ctx][2]
    with _engine(p0, ctx, monkeypatch) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, form)
        _rest(e, p0)
        _iterate(e, p0, ctx)
        _update(e, p1, new_rows, form)
        got = _iterate(e, p1, ctx)
    _same(got, _yardstick(p1, ctx, monkeypatch), (task, ctx))


# ---- 3. two updates in a row: the second buffers are swapped twice ------------------------------------------------------------
@pytest.mark.parametrize("task,ctx", [("acrobot", "fused"), ("acrobot", "fused_cols"), ("panda_reaching", "fused_w1"), ("panda_reaching", "records"),
                                      ("panda_pushing", "records_cols")])
def test_two_updates_in_a_row(task, ctx, monkeypatch):
    T, B = TASKS[task]
    p0 = _base(task)
    rows1 = {0: _bisected(task, T, 8100), 2: _every_step(task, T)}
    p1 = _merged(p0, rows1)
    rows2 = {1: _bisected(task, T, 8200), B - 1: _minimal(task, T)}
    p2 = _merged(p1, rows2)
    form = CONTEXTS[ctx][2]
    with _engine(p0, ctx, monkeypatch) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, form)
        _rest(e, p0)
        _iterate(e, p0, ctx)
        _update(e, p1, rows1, form)
        mid = _iterate(e, p1, ctx)
        _update(e, p2, rows2, form)
        got = _iterate(e, p2, ctx)
    _same(mid, _yardstick(p1, ctx, monkeypatch), "first update")
    _same(got, _yardstick(p2, ctx, monkeypatch), "second update")


# ---- 4. the pending state -----------------------------------------------------------------------------------------------------
def _raises(code, call, *a, **kw):
    with pytest.raises(KpilqrError) as ei:
        call(*a, **kw)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


@pytest.mark.parametrize("task,ctx", [("acrobot", "fused"), ("panda_reaching", "records"), ("panda_reaching", "fused_cols")])
def test_pending_ranges_refuse_every_reader_and_only_the_matching_upload_completes_them(task, ctx, monkeypatch):
    T, B = TASKS[task]
    p0 = _base(task)
    new_rows = _subsets(task)["pair"]
    traj = sorted(new_rows)
    p1 = _merged(p0, new_rows)
    form = CONTEXTS[ctx][2]
    other = "cols" if form == "fd_kp" else "fd_kp"
    want = _yardstick(p1, ctx, monkeypatch)
    with _engine(p0, ctx, monkeypatch) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        _payload(e, p0, form)
        _rest(e, p0)
        _iterate(e, p0, ctx)
        e.update_keypoints_rows(traj, [new_rows[b] for b in traj])
        _rest(e, p1)
        # every reader of the payload says what is missing
        for call in (lambda: e.iterate(p1["lam"], 100, ALPHAS), lambda: e.backward(p1["lam"]), e.fd_difference, e.interpolate, e.fd_interpolate,
                     e.get_AB, lambda: e.update_keypoints_rows(traj, [new_rows[b] for b in traj])):
            msg = _raises(ERR_STATE, call)
            assert "pending" in msg and "partial" in msg, msg
        if "fused" in ctx:
            _raises(ERR_STATE, e.backward_stats)
        # uploads that do not match are rejected and leave the state as it was
        _raises(ERR_ARG, _payload, e, p1, form, [traj[0]])                                   # another traj (and entries)
        _raises(ERR_ARG, _payload, e, p1, form, [traj[0], traj[1] + 1 if traj[1] + 1 < B else traj[1] - 1])
        xp, xm, md = synth.kp_ordered_payload(p1)
        idx = _entries_of(p1, traj)[:-1]                                                   # one entry short
        if form == "fd_kp":
            _raises(ERR_ARG, e.upload_fd_kp_partial, traj, e.fd_kp_slab(xp[idx], xm[idx], md[idx]), eps=p1["eps"])
            _raises(ERR_ARG, _payload, e, p1, form, traj, eps=np.nextafter(p1["eps"], 1.0))   # a context has one eps
        else:
            _raises(ERR_ARG, e.upload_kp_columns_partial, traj, e.kp_columns(xp[idx], xm[idx], md[idx], eps=p1["eps"]))
        _raises(ERR_STATE, _payload, e, p1, other, traj)                                     # the other payload kind
        _raises(ERR_STATE, e.iterate, p1["lam"], 100, ALPHAS)                                # still pending
        _payload(e, p1, form, traj)                                                          # the correct call still succeeds
        _same(_iterate(e, p1, ctx), want, "after rejected calls")
        # a whole upload clears the pending state at any time
        e.update_keypoints_rows(traj, [p0["kp_rows"][b] for b in traj])
        _raises(ERR_STATE, e.iterate, p0["lam"], 100, ALPHAS)
        _payload(e, p0, form)
        _rest(e, p0)
        back = _iterate(e, p0, ctx)
        # ... and so do new lists for everybody (the payload is dropped with them, as always)
        e.update_keypoints_rows(traj, [new_rows[b] for b in traj])
        e.set_keypoints_rows(p1["kp_rows"])
        _payload(e, p1, form)
        _rest(e, p1)
        _same(_iterate(e, p1, ctx), want, "after set_keypoints")
    _same(back, _yardstick(p0, ctx, monkeypatch), "after a whole upload")


def test_argument_checks():
    task = "acrobot"
    T, B = TASKS[task]
    p0 = _base(task)
    rows = _minimal(task, T)
    with Engine(p0["dof"], p0["m"], T, p0["nr"], batch=B, fused=True) as e:
        _raises(ERR_STATE, e.update_keypoints_rows, [0], [rows])                             # no lists yet
        e.set_keypoints_rows(p0["kp_rows"])
        for traj in ([1, 1], [2, 1], [-1, 0], [0, B]):                                       # strictly increasing, within [0, batch)
            _raises(ERR_ARG, e.update_keypoints_rows, traj, [rows, rows])
            _raises(ERR_ARG, e.gains, traj)
        o, t = rows_to_dof_csr([rows], p0["dof"], T)
        bad = t.copy(); bad[-1] = T
        _raises(ERR_ARG, e.update_keypoints, [0], o, bad)                                    # checked as set_keypoints checks
        down = o.copy(); down[1] = o[2] + 1
        _raises(ERR_ARG, e.update_keypoints, [0], down, np.zeros(down[-1], np.int32))
        # nothing of that changed the lists
        wo, wt = rows_to_dof_csr(p0["kp_rows"], p0["dof"], T)
        go, gt = e.get_keypoints()
        assert np.array_equal(go, wo) and np.array_equal(gt, wt)
        # without a payload there is nothing to carry and nothing pending
        e.update_keypoints_rows([0], [rows])
        p1 = _merged(p0, {0: rows})
        _payload(e, p1, "fd_kp")
        _rest(e, p1)
        e.iterate(p1["lam"], 100, ALPHAS)
        assert np.all(e.results()["status"] == 0)


@pytest.mark.parametrize("task,ctx", [("acrobot", "fused"), ("panda_reaching", "records")])
def test_job_list_payload_behaves_as_set_keypoints(task, ctx, monkeypatch):
    """Job lists carry their own indices: nothing is moved, nothing is pending, the context is what set_keypoints with the merged
    lists leaves.  (The listed trajectories shrink, so that every entry of the new lists still has its jobs.)"""
    T, B = TASKS[task]
    p0 = _base(task)
    new_rows = {0: _minimal(task, T), B - 1: _minimal(task, T)}
    traj = sorted(new_rows)
    merged = list(p0["kp_rows"])
    for b in traj:
        merged[b] = new_rows[b]
    out = []
    for how in ("update", "set"):
        with _engine(p0, ctx, monkeypatch) as e:
            e.set_keypoints_rows(p0["kp_rows"])
            e.upload_fd(p0["job_b"], p0["job_t"], p0["job_col"], p0["job_mode"], p0["xplus"], p0["xminus"], job_nom=p0["job_nom"], xnom=p0["xnom"],
                        eps=p0["eps"])
            _rest(e, p0)
            _iterate(e, p0, ctx)
            if how == "update":
                e.update_keypoints_rows(traj, [new_rows[b] for b in traj])
            else:
                e.set_keypoints_rows(merged)
            out.append(_iterate(e, p0, ctx))
            out[-1]["kp"] = np.concatenate(e.get_keypoints())
    assert np.all(out[0]["status"] == 0)
    _same(out[0], out[1], (task, ctx))


# ---- 5. lists placed on the device --------------------------------------------------------------------------------------------
def test_update_after_generate_keypoints_reads_the_offsets_back(monkeypatch):
    task, T, B = "panda_reaching", 60, 3
    _, cfg = synth._task_cfg(task)
    dof = cfg["dof"]
    rng = np.random.default_rng(T)
    X = np.stack([synth.contact_trajectory(rng, dof, T, cfg["dt"]) for _ in range(B)])
    for b in range(B):                        # velocity steps: key-points at different times per DoF
        for _ in range(2 * dof):
            X[b, int(rng.integers(2, T - 2)):, dof + int(rng.integers(0, dof))] += rng.uniform(-2, 2)
    gen = ("velocity_change", 2, 12, rng.uniform(0.5, 20.0, dof), cfg["dt"])
    with Engine(dof, cfg["m"], T, cfg["nr"], batch=B, fused=True) as e:
        e.upload_states(X); e.generate_keypoints(*gen)
        o, t = e.get_keypoints()
    rows = [synth.rows_from_dof_lists(dof, T, [t[o[b * dof + i]:o[b * dof + i + 1]] for i in range(dof)]) for b in range(B)]
    assert len(set(len(t[o[i]:o[i + 1]]) for i in range(dof))) > 1            # ragged indeed
    p0 = _problem(task, T, rows)
    new_rows = {1: _bisected(task, T, 31)}
    p1 = _merged(p0, new_rows)
    with Engine(dof, cfg["m"], T, cfg["nr"], batch=B, fused=True) as e:
        e.upload_states(X); e.generate_keypoints(*gen)      # the lists exist on the device only
        _payload(e, p0, "fd_kp")
        _rest(e, p0)
        _iterate(e, p0, "fused")
        _update(e, p1, new_rows, "fd_kp")
        go, gt = e.get_keypoints()
        got = _iterate(e, p1, "fused")
    wo, wt = rows_to_dof_csr(p1["kp_rows"], dof, T)
    assert np.array_equal(go, wo) and np.array_equal(gt, wt)
    _same(got, _yardstick(p1, "fused", monkeypatch), "generated lists")


# ---- 6. the gains of a subset -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,ctx", [("acrobot", "fused"), ("panda_pushing", "records")])
def test_partial_gains_download(task, ctx, monkeypatch):
    p = _base(task)
    B = p["batch"]
    with _engine(p, ctx, monkeypatch) as e:
        e.set_keypoints_rows(p["kp_rows"])
        _payload(e, p, "fd_kp")
        _rest(e, p)
        e.iterate(p["lam"], 100, ALPHAS)
        K, k = e.gains()
        assert np.any(K != 0) and np.any(k != 0)
        for traj in ([0], [B - 1], [0, 1], [0, B - 1], list(range(1, B)), list(range(B)), []):      # single ones, runs, a gap, everybody, nobody
            Kp, kp = e.gains(traj=traj)
            assert Kp.shape == (len(traj),) + K.shape[1:] and np.array_equal(Kp, K[traj]) and np.array_equal(kp, k[traj])
            Kp, none = e.gains(traj=traj, want_k=False)
            assert none is None and np.array_equal(Kp, K[traj])
            none, kp = e.gains(traj=traj, want_K=False)
            assert none is None and np.array_equal(kp, k[traj])


# ---- 7. the batch shim uses the route -----------------------------------------------------------------------------------------
def test_batched_optimiser_moves_fewer_bytes_than_whole_batch_transfers():
    """adaptive_accel on the six starts of tests/test_host.py's partial-regeneration test: a trajectory has a step rejected and
    carries on while the others regenerate.  Whole-batch transfers -- what the shim did before -- move exactly (linearisations x the
    batch's payload) up and (iterations x B x a trajectory's gains) down."""
    q0s = np.array([[3.1415, 0.3], [2.6, -0.4], [3.5, 0.1], [1.2, 0.8], [0.4, -1.1], [2.9, 0.9]])
    T, n, m = 120, 4, 1
    res = host.run_acrobot_batch(q0s, T=T, min_N=3, max_iter=9, min_iter=2, torque_weight=1e-3, fused=True, method="adaptive_accel")
    entries = res["keypoint_entries"]
    assert len(entries) >= 2 and np.all(entries > 0)
    whole_up = int(entries.sum()) * (6 * n + 2) * 8
    whole_down = int(res["iterations"].max()) * len(q0s) * (T * n * m + T * m) * 8
    print(f"payload up {res['payload_bytes_uploaded']} of {whole_up} bytes, gains down {res['gain_bytes_downloaded']} of {whole_down} bytes")
    assert 0 < res["payload_bytes_uploaded"] < whole_up
    assert 0 < res["gain_bytes_downloaded"] < whole_down
