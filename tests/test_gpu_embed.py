"""KPILQR_FLAG_EMBED_SHAPE on the device: one-tile shapes without kernels of their own run the fused sweeps of their carrier shape.

Every case runs the SAME caller's problem three ways and holds them against each other:
  (a) the embedded context reports the fused variant, the ":emb<n'>x<m'>" suffix and the carrier tests/_embed.py predicts -- on a
      library without the feature the flag is ignored and the shape runs the tiled or generic kernels;
  (b) K, k, delta_J, cost_pred and U_alpha are within 1e-9 (relative to the array's max) of the CPU oracle run on the CALLER's
      shape, status equal;
  (c) they are BIT-IDENTICAL to a context created natively at the carrier's shape and fed the host-padded problem of
      tests/_embed.py, restricted to the real block: the same kernels on the same input bits, so this isolates the embedding and
      extraction kernels (embed.hip);
  (d) gains(f32=True) is the float cast of (c)'s K, bit for bit.
B = 3 distinct trajectories; T = 23 with pd_check_stride 5 and T = 130 with the default 100; uniform and per-DoF lists; the key-point
ordered payload (one-sided fraction 0.1: the mode bits matter) and the column payload; constant and per-step residual Jacobians;
the library's wave forms for 3 trajectories and the one-wave forms (KPILQR_FUSED_WAVES = KPILQR_FUSED_FWD_WAVES = 1)."""
import functools

import numpy as np
import pytest

import _embed as E
import _shapes as S
from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import Engine, _lib, synth
from trajoptkp_amd.engine import KpilqrError

pytestmark = pytest.mark.gpu

RTOL = 1e-9
B = 3
SHAPES = ((6, 6, 9), (3, 2, 5), (1, 1, 3), (6, 2, 4), (7, 3, 6))          # (dof, m, nr)
HORIZONS = ((23, 5), (130, 100))                                         # (T, pd_check_stride); key-points every 5 steps
COMBOS = [(lists, payload, rxc) for lists in ("uni", "ragged") for payload in ("kp", "cols") for rxc in (True, False)]
ONE_WAVE = {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}
# every (shape, horizon, lists, payload, Jacobians); the wave form alternates so that every combination of lists, payload and
# Jacobians runs in both forms (one per horizon) on every shape
CASES = [(shape, hz, combo, bool((ci + hi) % 2)) for shape in SHAPES for hi, hz in enumerate(HORIZONS) for ci, combo in enumerate(COMBOS)]


def _id(case):
    (dof, m, nr), (T, pd), (lists, payload, rxc), w1 = case
    return f"d{dof}m{m}r{nr}-T{T}-{lists}-{payload}-{'rxc' if rxc else 'rx'}-{'w1' if w1 else 'auto'}"


@functools.lru_cache(maxsize=None)
def _problem(dof, m, nr, T, lists, rxc, config_id=4):
    task = synth.shape_task(dof, m, nr)
    if lists == "uni":
        return synth.make_problem(task=task, T=T, batch=B, min_N=5, dense_residuals=not rxc, one_sided_frac=0.1, config_id=config_id)
    rng = np.random.default_rng(1000 * dof + m)
    rows = [synth.bisect_keypoints(rng, dof, T, 2, np.linspace(0.0, 1.0, dof)) for _ in range(B)]
    return synth.make_ragged_problem(task, T, rows, config_id=config_id, dense_residuals=not rxc, one_sided_frac=0.1)


@functools.lru_cache(maxsize=None)
def _oracle(dof, m, nr, T, lists, rxc, pd, lam=None):
    p = _problem(dof, m, nr, T, lists, rxc)
    return tuple(pipeline.run_trajectory(p, b, lam=lam, pd_stride=pd, want_U=True) for b in range(B))


def _set_env(monkeypatch, env):
    for key in S.ENV_KEYS + ("KPILQR_FUSED_RAW", "KPILQR_FUSED_UNI"):
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)


def _upload(e, p, payload, rxc):
    e.set_keypoints_rows(p["kp_rows"])
    xp, xm, mode = synth.kp_ordered_payload(p)
    if payload == "kp":
        e.upload_fd_kp(e.fd_kp_slab(xp, xm, mode), eps=p["eps"])
    else:
        e.upload_kp_columns(e.kp_columns(xp, xm, mode, eps=p["eps"]))
    if rxc:
        e.upload_residuals(p["r"], None, None, p["w_run"], p["w_term"])
        e.upload_residual_jacobians_const(p["rx_const"], None)
    else:
        e.upload_residuals(p["r"], p["r_x"], p["r_u"] if np.any(p["r_u"]) else None, p["w_run"], p["w_term"])
    e.upload_nominal(p["u_nom"], p["ctrl_lim"])
    e.sync()


def _run(p, payload, rxc, pd, lam=None, embed=False, n_alpha=6):
    """One iteration of problem p on a fused context of p's shape -> everything the assertions look at."""
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], n_alpha=n_alpha, fused=True, embed=embed) as e:
        _upload(e, p, payload, rxc)
        e.iterate(p["lam"] if lam is None else lam, pd, orc.alphas(n_alpha))
        res = e.results()
        K, k = e.gains()
        K32, _ = e.gains(f32=True, want_k=False)
        cost, U = e.forward_linear(None, want_U=True)
        try:
            carrier = e.carrier_dims()
        except KpilqrError as err:
            assert err.code == _lib.ERR_STATE
            carrier = None
        return dict(status=res["status"], delta_J=res["delta_J"], cost_pred=res["cost_pred"], cost=cost, K=K, k=k, K32=K32, U=U,
                    carrier=carrier, variants=(e.backward_variant, e.forward_variant),
                    launch=(e.last_launch("backward"), e.last_launch("forward")))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def _check_oracle(g, refs, tag, dj_by_cost=False):
    """dj_by_cost: delta_J is held to RTOL of the predicted costs' magnitude instead of its own -- for lambda = 0, where it is
    sum_t (k'Q_u + k'Q_uu k) with k = -Q_uu^-1 Q_u, i.e. EXACTLY 0 in exact arithmetic: both sides return the rounding noise of
    terms of the size of k'Q_u, and the predicted cost change is a sum of those same terms."""
    for b, o in enumerate(refs):
        assert g["status"][b] == o["status"], (tag, b, g["status"][b], o["status"])
        if o["status"] != 0:
            continue
        errs = dict(K=_rel(g["K"][b], o["K"]), k=_rel(g["k"][b], o["k"]),
                    delta_J=abs(g["delta_J"][b] - o["delta_J"]) / max(float(np.max(np.abs(o["cost_pred"]))) if dj_by_cost else abs(o["delta_J"]), 1e-300),
                    cost=_rel(g["cost_pred"][b], o["cost_pred"]), U=_rel(g["U"][b], o["U_alpha"]))
        assert max(errs.values()) <= RTOL, (tag, b, g["launch"], errs)


def _check_carrier_bits(g, nat, dof, m, cdof, tag):
    real = E.real_block(nat, dof, m, cdof)
    assert np.array_equal(g["status"], nat["status"]), (tag, g["status"], nat["status"])
    for key in ("K", "k", "delta_J", "cost_pred", "cost", "U"):
        assert _same_bits(g[key], real[key]), (tag, key)
    ok = nat["status"] == 0
    assert not np.any(real["K_pad"].reshape(B, -1)[ok]) and not np.any(real["k_pad"].reshape(B, -1)[ok]), tag      # the padded gains are exactly 0
    with np.errstate(over="ignore"):
        assert _same_bits(g["K32"], real["K"].astype(np.float32)), (tag, "K32")


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_embedded_shape(case, monkeypatch):
    (dof, m, nr), (T, pd), (lists, payload, rxc), w1 = case
    cd = E.embedded(dof, m, nr, T, 6, S.FLAG_FUSED | E.FLAG_EMBED)
    assert cd == E.carrier(dof, m) and cd is not None
    p = _problem(dof, m, nr, T, lists, rxc)
    _set_env(monkeypatch, ONE_WAVE if w1 else {})
    g = _run(p, payload, rxc, pd, embed=True)
    nat = _run(E.pad_problem(p, *cd), payload, rxc, pd)
    tag = _id(case)
    # (a) the fast path, and the carrier the model predicts
    assert g["variants"] == ("mfma_f64_t1_fused", "mfma_f64_t1_fused"), g["variants"]
    assert g["carrier"] == cd, (g["carrier"], cd)
    sfx = f":emb{2 * cd[0]}x{cd[1]}"
    assert nat["carrier"] is None and all(":emb" not in s for s in nat["launch"])
    assert g["launch"] == tuple(s + sfx for s in nat["launch"]), (g["launch"], nat["launch"])       # the carrier's form, suffix last
    if w1:
        assert all(":w1:" in s for s in g["launch"]), g["launch"]
        uni = lists == "uni" or dof == 1
        assert (":raw:" in g["launch"][0]) == (payload == "kp" and uni), g["launch"]
        if rxc and uni:                                  # the padded constant Jacobian is kept in registers, as on the carrier
            assert all(s.endswith(":uni:ru0:rxc" + sfx) for s in g["launch"]), g["launch"]
    # (b) the caller's problem on the CPU oracle
    _check_oracle(g, _oracle(dof, m, nr, T, lists, rxc, pd), tag)
    # (c), (d) the carrier's own bits
    _check_carrier_bits(g, nat, dof, m, cd[0], tag)


def test_lambda_rule(monkeypatch):
    _set_env(monkeypatch, {})
    p = _problem(6, 6, 9, 23, "uni", True)
    with Engine(6, 6, 23, 9, batch=B, fused=True, embed=True) as e:
        _upload(e, p, "kp", True)
        for lam in (0.0, [0.1, -1.0, 0.1], [0.1, 0.1, float("nan")]):
            for call in (lambda: e.backward(lam, 5), lambda: e.iterate(lam, 5, orc.alphas(6))):
                with pytest.raises(KpilqrError) as ei:
                    call()
                assert ei.value.code == _lib.ERR_ARG and "lambda I" in str(ei.value), str(ei.value)
        st, _ = e.backward(0.1, 5)                       # (nothing was enqueued or changed: the context works on)
        assert not np.any(st)
        st, _ = e.backward(None, 5)                      # lambda = NULL: the resident lambdas
        assert not np.any(st)
    # m' == m: lambda = 0 is legal and agrees with the oracle at lambda = 0
    q = _problem(1, 1, 3, 130, "uni", False)
    refs = _oracle(1, 1, 3, 130, "uni", False, 100, 0.0)
    assert all(o["status"] == 0 for o in refs)
    g = _run(q, "kp", False, 100, lam=0.0, embed=True)
    assert g["carrier"] == (2, 1)
    _check_oracle(g, refs, "lambda0-d1m1", dj_by_cost=True)


def test_lambda_retry_as_on_the_carrier(monkeypatch):
    """Negated running weights (tests/_lambda_retry.py): first attempts fail, the device raises lambda per trajectory."""
    _set_env(monkeypatch, ONE_WAVE)
    p = dict(synth.make_problem(task=synth.shape_task(6, 6, 9), T=48, batch=B, min_N=5, dense_residuals=True, config_id=4))
    p["w_run"] = -(np.abs(p["w_run"]) + 1.0) * 2.0
    lam0 = np.array([0.1, 1.0, 1e-4])
    first = [pipeline.run_trajectory(p, b, lam=lam0[b], pd_stride=10, stages=("fd", "interp", "cost", "bwd"))["status"] for b in range(B)]
    assert first[0] != 0 and first[1] == 0 and first[2] != 0             # (the oracle: what the first attempt of each does)
    out = []
    for q, embed in ((p, True), (E.pad_problem(p, 7, 7), False)):
        with Engine(q["dof"], q["m"], q["T"], q["nr"], batch=B, fused=True, embed=embed) as e:
            _upload(e, q, "kp", False)
            e.set_lambda_retry(10.0, 10.0, 6)
            st, dJ = e.backward(lam0, 10)
            used, att = e.lambda_retry()
            K, k = e.gains()
            out.append(dict(status=st, delta_J=dJ, used=used, att=att, K=K, k=k))
    g, nat = out
    assert np.array_equal(g["att"], nat["att"]) and _same_bits(g["used"], nat["used"]) and np.array_equal(g["status"], nat["status"])
    assert g["att"][0] > 1 and g["att"][1] == 1 and g["att"][2] > 1, g["att"]
    real = E.real_block(nat, 6, 6, 7)
    ok = g["status"] == 0
    assert ok.any() and _same_bits(g["K"][ok], real["K"][ok]) and _same_bits(g["k"][ok], real["k"][ok]) and _same_bits(g["delta_J"][ok], nat["delta_J"][ok])


def test_refused_calls_leave_the_context_alone(monkeypatch):
    _set_env(monkeypatch, {})
    p = _problem(3, 2, 5, 23, "ragged", False)
    with Engine(3, 2, 23, 5, batch=B, fused=True, embed=True) as e:
        _upload(e, p, "cols", False)

        def once():
            e.iterate(p["lam"], 5, orc.alphas(6))
            res = e.results()
            K, k = e.gains()
            return dict(res, K=K, k=k, launch=(e.last_launch("backward"), e.last_launch("forward")))
        before = once()
        refused = (("kpilqr_fd_difference", lambda: e.fd_difference()), ("kpilqr_get_AB", lambda: e.get_AB()),
                   ("kpilqr_backward_stats", lambda: e.backward_stats(5)), ("kpilqr_download_gains_partial", lambda: e.gains(traj=[0])),
                   ("kpilqr_backward_partial", lambda: e.backward_partial([0, 2], 0.1, 5)), ("kpilqr_resize", lambda: e.resize(2, 1, 23)))
        for name, call in refused:
            with pytest.raises(KpilqrError) as ei:
                call()
            assert ei.value.code == _lib.ERR_STATE and name in str(ei.value) and "not on an embedded context" in str(ei.value), (name, str(ei.value))
        assert (e.dof, e.m) == (3, 2)
        after = once()
        for key in ("status", "delta_J", "cost_pred", "K", "k"):
            assert _same_bits(before[key], after[key]), key
        assert before["launch"] == after["launch"]


def test_flag_is_ignored_on_a_compiled_shape(monkeypatch):
    _set_env(monkeypatch, {})
    p = _problem(7, 7, 9, 23, "uni", True)
    assert E.embedded(7, 7, 9, 23, 6, S.FLAG_FUSED | E.FLAG_EMBED) is None
    g = _run(p, "kp", True, 5, embed=True)
    h = _run(p, "kp", True, 5, embed=False)
    assert g["carrier"] is None and g["variants"] == h["variants"] and g["launch"] == h["launch"]
    assert all(":emb" not in s for s in g["launch"])
    for key in ("status", "delta_J", "cost_pred", "cost", "K", "k", "K32", "U"):
        assert _same_bits(g[key], h[key]), key
