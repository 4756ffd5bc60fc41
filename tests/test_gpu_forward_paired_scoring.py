"""The paired scoring of the uniform one-wave forward sweep with a constant residual Jacobian (forward_fused_body, P2: one r_x
product scores two steps while n_alpha <= 8) against the CPU oracle and against the forms that score every step by itself.

Every case is B = 3 on a fused context with the key-point ordered payload and the task's constant Jacobian; the one-wave forms are
forced (the batch would pick the wave pairs).  Each asserts the form that ran (":w1:uni:ru0:rxc"), what
last_launch("forward_scoring") says of it, and status 0 on both sides.  Bars: 1e-9 relative to the oracle for cost_pred and
U_alpha (the project's bar for every sweep), 1e-12 relative between two GPU forms (the bar of the constant-Jacobian sister forms)."""
import numpy as np
import pytest

import _clamp
import _shapes as S
from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import Engine, synth

pytestmark = pytest.mark.gpu

RTOL, RTOL_FORMS = 1e-9, 1e-12
B = 3
SHAPES = ((7, 7), (6, 3), (5, 3), (2, 1))                  # (dof, m) of the four one-tile shapes, S.T1_SHAPES
ODD_NR = {7: 5, 6: 3, 5: 5, 2: 3}                           # an odd residual count per shape: the pair fetch's over-read meets the row offset
FORM = ":w1:uni:ru0:rxc"


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def _one_wave(monkeypatch):
    for key in S.ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("KPILQR_FUSED_WAVES", "1"); monkeypatch.setenv("KPILQR_FUSED_FWD_WAVES", "1")


def _problem(dof, m, nr, T, min_N, config_id=4):
    return synth.make_problem(task=synth.shape_task(dof, m, nr), T=T, batch=B, min_N=min_N, one_sided_frac=0.1, config_id=config_id)


def _gpu(p, n_alpha, rx_const=True, want_U=False):
    """Backward + forward over the alphas on a fused context (the environment is read at creation: _one_wave first)."""
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=B, n_alpha=n_alpha, fused=True) as e:
        fresh = e.last_launch("forward_scoring")
        synth.upload(e, p, kp_ordered=True, rx_const=rx_const)
        st, _ = e.backward(p["lam"], 100)
        out = e.forward_linear(orc.alphas(n_alpha), want_U=want_U)
        cost, U = out if want_U else (out, None)
        return dict(status=st, cost=cost, U=U, fresh=fresh, form=e.last_launch("forward"), scoring=e.last_launch("forward_scoring"))


def _refs(p, n_alpha, want_U=False):
    refs = [pipeline.run_trajectory(p, b, n_alpha=n_alpha, want_U=want_U) for b in range(B)]
    assert all(o["status"] == 0 for o in refs)
    return refs


def _hold(g, refs, scoring, tag, with_U=False, form=FORM):
    assert g["form"].endswith(form), (tag, g["form"])
    assert g["scoring"] == scoring, (tag, g["scoring"])
    assert list(g["status"]) == [0] * B, (tag, list(g["status"]))
    for b, o in enumerate(refs):
        err = _rel(g["cost"][b], o["cost_pred"])
        assert err <= RTOL, (tag, b, "cost_pred", err)
        if with_U:
            err = _rel(g["U"][b], o["U_alpha"])
            assert err <= RTOL, (tag, b, "U_alpha", err)


# ---- 1. every residue of the four-step group below, at and above one group; crossings on even and on odd members; both residual counts
@pytest.mark.parametrize("dof,m", SHAPES, ids=[f"d{d}m{m}" for d, m in SHAPES])
@pytest.mark.parametrize("T", range(2, 14))
def test_horizons_and_parities(T, dof, m, monkeypatch):
    _one_wave(monkeypatch)
    for min_N in (1, 2, 3, 5):
        for nr in (2 * dof, ODD_NR[dof]):
            p = _problem(dof, m, nr, T, min_N)
            _hold(_gpu(p, 6), _refs(p, 6), "pair2", (T, dof, m, min_N, nr))


# ---- 2. the n_alpha rule: pairs while the candidates fill at most half of the tile
@pytest.mark.parametrize("dof,m", ((7, 7), (2, 1)), ids=("d7m7", "d2m1"))
@pytest.mark.parametrize("T", (9, 10))
@pytest.mark.parametrize("n_alpha,scoring", ((1, "pair2"), (2, "pair2"), (6, "pair2"), (8, "pair2"), (9, "step"), (16, "step")))
def test_alpha_counts(n_alpha, scoring, T, dof, m, monkeypatch):
    assert S.fused_supported(2 * dof, m, 9, dof, T, 16) and not S.fused_supported(2 * dof, m, 9, dof, T, 17)     # 16: the largest
    _one_wave(monkeypatch)
    p = _problem(dof, m, 9 if dof == 7 else 4, T, 2)
    _hold(_gpu(p, n_alpha), _refs(p, n_alpha), scoring, (n_alpha, T, dof, m))


# ---- 3. the idle columns (c >= n_alpha roll out alpha = 0) carry a non-zero state once a nominal control lies outside its limits
CLAMP_SEED = 4          # config_id of the problem and
CLAMP_OUT = 0.25        # how far outside (in units of the limit interval): chosen on the oracle, see clamp_problem


def clamp_problem(T, n_alpha, dof=7, m=7, nr=9):
    """An activated clamp case (_clamp.activate) whose nominal control t mod m of step t is then moved outside its limits, above on
    even steps and below on odd ones: alpha = 0 no longer reproduces the nominal controls, so every column of the tile, used or
    idle, rolls out a non-zero state.  Returns the problem and the oracle's linearisation."""
    p = _problem(dof, m, nr, T, 2, config_id=CLAMP_SEED)
    lin = _clamp.linearise(p)
    q = _clamp.activate(p, n_alpha, lin, q=(0.1, 0.9))
    _clamp.assert_conditions(_clamp.conditions(q, n_alpha, lin), n_alpha, "activated")
    lo, hi = q["ctrl_lim"][0::2], q["ctrl_lim"][1::2]
    u = q["u_nom"].copy()
    for t in range(T):
        j = t % m
        u[:, t, j] = hi[j] + CLAMP_OUT * (hi[j] - lo[j]) if t % 2 == 0 else lo[j] - CLAMP_OUT * (hi[j] - lo[j])
    q = dict(q, u_nom=u)
    return q, lin


@pytest.mark.parametrize("n_alpha", (6, 8))
@pytest.mark.parametrize("T", (12, 13))
def test_idle_columns_do_not_leak(T, n_alpha, monkeypatch):
    q, lin = clamp_problem(T, n_alpha)
    cond = _clamp.conditions(q, n_alpha, lin)            # on the oracle, before any GPU run
    print("clamp case", T, n_alpha, {k: v for k, v in cond.items() if k != "cost"})
    _clamp.assert_conditions(cond, n_alpha, (T, n_alpha))
    assert cond["ran"] == B
    outside = (q["u_nom"] > q["ctrl_lim"][1::2]) | (q["u_nom"] < q["ctrl_lim"][0::2])
    assert np.all(outside.sum(axis=2) >= 1)              # one nominal control of every step
    refs = _clamp.references(q, n_alpha, lin)
    assert all(o["status"] == 0 for o in refs)
    _one_wave(monkeypatch)
    _hold(_gpu(q, n_alpha, want_U=True), refs, "pair2", (T, n_alpha), with_U=True)


# ---- 4. negative running and terminal weights: the sign joins behind the sum of the two half-sums, so both parities of T
@pytest.mark.parametrize("T", (9, 10))
def test_negative_weights(T, monkeypatch):
    _one_wave(monkeypatch)
    p = synth.make_problem(task="panda_reaching", T=T, batch=B, min_N=5, lam=1.0)
    p["w_run"] = p["w_run"].copy(); p["w_term"] = p["w_term"].copy()
    p["w_run"][[2, 9]] *= -0.05
    p["w_term"][[4]] *= -0.01
    _hold(_gpu(p, 6), _refs(p, 6), "pair2", T)


# ---- 5. against the form that scores every step by itself (the same Jacobian given per step)
@pytest.mark.parametrize("T", (13, 131))
def test_against_the_per_step_form(T, monkeypatch):
    _one_wave(monkeypatch)
    p = synth.make_problem(task="panda_reaching", T=T, batch=B, min_N=5)
    a = _gpu(p, 6)
    b = _gpu(p, 6, rx_const=False)
    assert a["form"].endswith(FORM) and a["scoring"] == "pair2", (a["form"], a["scoring"])
    assert b["form"].endswith(":w1:uni:ru0") and b["scoring"] == "step", (b["form"], b["scoring"])
    assert list(a["status"]) == list(b["status"]) == [0] * B
    err = float(np.max(np.abs(a["cost"] - b["cost"]))) / float(np.max(np.abs(b["cost"])))
    print("paired against per-step", T, err)
    assert err <= RTOL_FORMS, (T, err)


# ---- 6. the listed twin takes the same path
def test_listed_sweep(monkeypatch):
    _one_wave(monkeypatch)
    p = _problem(7, 7, 9, 13, 3)
    a1, a2 = orc.alphas(6), orc.alphas(6) * 0.5
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=B, n_alpha=6, fused=True) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=True)
        st, _ = e.backward(p["lam"], 100)
        assert list(st) == [0] * B
        c1 = e.forward_linear(a1)
        cp, Up = e.forward_linear_partial([0, 2], a2, want_U=True)
        form_p, scoring_p = e.last_launch("forward"), e.last_launch("forward_scoring")
        res = e.results()["cost_pred"]
        c2, U2 = e.forward_linear(a2, want_U=True)
        form_w, scoring_w = e.last_launch("forward"), e.last_launch("forward_scoring")
    assert form_w.endswith(FORM) and form_p == form_w + ":subset", (form_p, form_w)
    assert scoring_p == scoring_w == "pair2", (scoring_p, scoring_w)
    assert np.array_equal(res[1], c1[1]) and not np.array_equal(c1[1], c2[1])        # the unlisted row: untouched
    assert np.array_equal(res[[0, 2]], cp)
    assert np.array_equal(cp, c2[[0, 2]]) and np.array_equal(Up, U2[[0, 2]])          # the listed rows: bit for bit the whole-batch call's


# ---- 7. nothing launched, nothing said
def test_fresh_context_reports_nothing(monkeypatch):
    _one_wave(monkeypatch)
    from trajoptkp_amd.engine import KpilqrError
    with Engine(7, 7, 9, 9, batch=B, fused=True) as e:
        assert e.last_launch("forward_scoring") == ""
        with pytest.raises(KpilqrError):                         # refused before its launch (no key-points yet): still nothing launched
            e.forward_linear(orc.alphas(6), fetch=False)
        assert e.last_launch("forward_scoring") == ""
        p = _problem(7, 7, 9, 9, 2)
        synth.upload(e, p, kp_ordered=True, rx_const=True)
        e.backward(p["lam"], 100)
        assert e.last_launch("forward_scoring") == ""            # a backward sweep is no forward launch


# ---- 8. a context that has only ever run streamed iterations: the chunks' forward launches are the context's last forward launch
@pytest.mark.parametrize("nchunks", (1, 2))
def test_streamed_iteration_reports_its_scoring(nchunks, monkeypatch):
    """kpilqr_iterate_streamed runs its sweeps on per-chunk views of the context; what they launched has to come back with the
    plan.  No forward call is made here but the chunks' own (the resident alphas are the zeros the context starts with: the strings
    and the status are what this case is about)."""
    _one_wave(monkeypatch)
    p = _problem(7, 7, 9, 13, 3)
    xp, xm, mode = synth.kp_ordered_payload(p)
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=B, n_alpha=6, fused=True) as e:
        e.set_keypoints_rows(p["kp_rows"])
        e.upload_residuals(None, None, None, p["w_run"], p["w_term"])
        e.upload_residual_jacobians_const(p["rx_const"], None)
        e.upload_nominal(None, p["ctrl_lim"])
        assert e.last_launch("forward_scoring") == ""
        pin = {}
        for name in ("r", "u_nom"):
            pin[name] = e.pinned(p[name].shape); pin[name][...] = p[name]
        lam = e.pinned(B); lam[:] = p["lam"]
        cp = e.pinned((B, 6)); st = e.pinned(B, np.int32); st[:] = -1
        e.iterate_streamed(fd_kp=e.fd_kp_slab(xp, xm, mode), eps=p["eps"], lam=lam, cost_pred=cp, status=st, nchunks=nchunks, **pin)
        e.sync()
        form, scoring = e.last_launch("forward"), e.last_launch("forward_scoring")
    assert list(st) == [0] * B, list(st)
    assert form.endswith(FORM), form
    assert scoring == "pair2", scoring
