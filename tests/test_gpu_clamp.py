"""The control clamp of every forward-sweep instantiation against the CPU oracle.  The cases of tests/test_gpu_shapes.py, with
the inputs of tests/_clamp.activate: about 30 % of the controls of every alpha on a limit, on both limits of every control,
limits that differ per control and cut into u_nom itself (tests/test_clamp_cases.py holds the cases to that on the oracle).  On
top of the parity of test_gpu_shapes (same RTOL, same dispatch assertion) every control of the device lies inside its limits
with no tolerance, and every entry the oracle puts on a limit is on it on the device."""
import numpy as np
import pytest

import _clamp
import _shapes as S
from _shape_run import (RTOL, _backward, _case_id, _check, _check_dispatch, _engine, _errs, _launched, _n_simd, _problem, _rel, _run,
                        _set_env, _take)
from oracle import oracle as orc
from trajoptkp_amd import Engine, synth

pytestmark = pytest.mark.gpu

_CASES = [c for c in S.cases(1024) if c["why"] != "refused"]


def _kp_ordered(c):
    return bool(c["flags"] & S.FLAG_FUSED) and (c["dof"] + c["nr"]) % 2 == 1     # both payload forms over the fused cases


def _check_limits(U, o, lim, tag):
    """U [n_alpha, T, m] of the device inside the limits exactly, and on them (to RTOL of the controls' magnitude, the measure of
    the parity check: an entry the device leaves a rounding error short of its limit is not clamped there) where the oracle's are."""
    lo, hi = lim[0::2], lim[1::2]
    assert np.all(U >= lo) and np.all(U <= hi), (tag, float(np.max(lo - U)), float(np.max(U - hi)))
    tol = RTOL * float(np.max(np.abs(o["U_alpha"])))
    for bound in (lo, hi):
        on = o["U_alpha"] == bound
        assert np.all(np.abs(U - bound)[on] <= tol), (tag, float(np.max(np.abs(U - bound)[on])), tol)


def _check_clamped(c, g, refs, p, rows, tag):
    _check(g, refs, rows, tag)
    worst = dict(U=0.0, cost=0.0)
    for b in rows:
        o = refs[b % len(refs)]
        if o["status"] == 0:
            _check_limits(g["U"][b], o, p["ctrl_lim"], (tag, b))
            e = _errs(g, o, b)
            worst = {k: max(worst[k], e[k]) for k in worst}
    return worst


def _report(c, cond, worst, tag):
    fwd = S.case_keys(c, _n_simd())[1]
    print(f"clamp_parity {fwd[0]} {tag} share={cond['share']:.3f} hits={min(cond['hits_lo'], cond['hits_hi'])} differ={cond['differ']} "
          f"U={worst['U']:.2e} cost={worst['cost']:.2e}")


@pytest.mark.parametrize("c", _CASES, ids=[_case_id(c) for c in _CASES])
def test_shape_clamped_matches_oracle(c, monkeypatch):
    n_simd = _n_simd()
    p0 = _problem(c)
    lin = _clamp.linearise(p0)
    p = _clamp.activate(p0, c["n_alpha"], lin)
    cond = _clamp.conditions(p, c["n_alpha"], lin)
    _clamp.assert_conditions(cond, c["n_alpha"], _case_id(c))
    g = _run(c, p, monkeypatch, kp_ordered=_kp_ordered(c))
    _check_dispatch(c, g, n_simd)
    refs = _clamp.references(p, c["n_alpha"], lin)
    assert all(o["status"] == 0 for o in refs) or c["why"] == "long"
    worst = _check_clamped(c, g, refs, p, range(p["batch"]), _case_id(c))
    _report(c, cond, worst, _case_id(c))


def test_clamped_batch_boundaries(monkeypatch):
    """n_simd + 1 trajectories: the plain twins of the one-tile and the one-wave fused forward, and the plain one-tile forward with
    two control chunks.  7 distinct trajectories, activated and then tiled, every one of the batch checked against its oracle."""
    n_simd = _n_simd()
    for c in S.batch_cases(n_simd):
        if c["batch"] != n_simd + 1:
            continue
        c = dict(c, T=17)
        base0 = _problem(c, batch=7, config_id=5)
        lin = _clamp.linearise(base0)
        base = _clamp.activate(base0, c["n_alpha"], lin)
        cond = _clamp.conditions(base, c["n_alpha"], lin)
        _clamp.assert_conditions(cond, c["n_alpha"], _case_id(c))
        refs = _clamp.references(base, c["n_alpha"], lin)
        p = _take(synth.tile_problem(base, -(-c["batch"] // 7)), c["batch"])
        g = _run(c, p, monkeypatch, kp_ordered=bool(c["flags"] & S.FLAG_FUSED))
        _check_dispatch(c, g, n_simd)
        assert "plain" in S.case_keys(c, n_simd)[1], c
        worst = _check_clamped(c, g, refs, p, range(c["batch"]), _case_id(c))
        _report(c, cond, worst, _case_id(c))


# one case per forward family, the smallest that reaches it: (forward key prefix, case)
_A6 = S.TILED_ENVS["a6"]
_EDGE = [(("t1_fwd", 4, 2), S._case(7, 7, 4, 0, why="edge")),
         (("fused_fwd", 4, 2, "pair"), S._case(7, 7, 4, S.FLAG_FUSED, {"KPILQR_FUSED_FWD_WAVES": "4"}, rx_const=True, why="edge")),
         (("fused_fwd", 4, 2, "triple"), S._case(7, 7, 4, S.FLAG_FUSED, {"KPILQR_FUSED_FWD_WAVES": "3"}, rx_const=True, why="edge")),
         (("tiled_fwd", 2, "-"), S._case(12, 7, 4, 0, S.TILED_ENVS["no_fsc"], why="edge")),
         (("tiled_fwd_sc",), S._case(12, 7, 4, 0, why="edge")),
         (("tiled_fwd", 2, "a6"), S._case(12, 7, 4, S.FLAG_FUSED, _A6, rx_const=True, why="edge")),
         (("wide_fwd", 2), S._case(12, 17, 5, 0, why="edge")),
         (("generic_fwd",), S._case(7, 7, 4, 0, n_alpha=17, why="edge"))]


@pytest.mark.parametrize("key,c", _EDGE, ids=["-".join(str(x) for x in key) for key, _ in _EDGE])
def test_clamp_edge_limits(key, c, monkeypatch):
    """Control 0 pinned (lo = hi), the last control unlimited at +-1e300 -- the kernels' own pad sentinel, which on a real control
    means no limit --, control m - 2 limited from above only."""
    n_simd = _n_simd()
    assert S.case_keys(c, n_simd)[1][:len(key)] == key
    m, na = c["m"], c["n_alpha"]
    p0 = _problem(c)
    lin = _clamp.linearise(p0)
    p = _clamp.edge_limits(_clamp.activate(p0, na, lin), na, lin)
    lim = p["ctrl_lim"]
    assert lim[0] == lim[1] and lim[2 * m - 2] == -1e300 and lim[2 * m - 1] == 1e300 and lim[2 * m - 4] == -1e300 < lim[2 * m - 3] < 1e30
    refs = _clamp.references(p, na, lin)
    assert all(o["status"] == 0 for o in refs)
    Uo = np.stack([o["U_alpha"] for o in refs])
    assert np.all(Uo[..., 0] == lim[0]) and np.sum(Uo[..., m - 2] == lim[2 * m - 3]) >= 2        # (the oracle pins, and hits the upper limit)
    assert np.sum(Uo[..., 1:m - 2] == lim[2:2 * m - 4:2]) >= 2 and np.sum(Uo[..., 1:m - 2] == lim[3:2 * m - 4:2]) >= 2
    g = _run(c, p, monkeypatch, kp_ordered=_kp_ordered(c))
    _check_dispatch(c, g, n_simd)
    _check_clamped(c, g, refs, p, range(p["batch"]), key)
    assert np.all(g["U"][..., 0] == lim[0])                                     # bit-equal to the pinned value
    assert np.all(np.abs(g["U"][..., m - 1]) < 1e30)                            # never on a limit


_LIVE = [_EDGE[0][1], S._case(7, 7, 4, S.FLAG_FUSED, rx_const=True, why="live"), _EDGE[4][1], _EDGE[6][1]]


@pytest.mark.parametrize("c", _LIVE, ids=["t1", "fused", "tiled_sc", "wide"])
def test_limits_and_nominal_replaced_on_a_live_context(c, monkeypatch):
    """The limits and the nominal controls are read fresh at every launch of the forward sweep, and a clamping run leaves nothing
    behind: wide limits, new limits, new nominal controls, and the first inputs again on ONE context."""
    n_simd = _n_simd()
    na = c["n_alpha"]
    al = orc.alphas(na)
    p = _problem(c)
    lin = _clamp.linearise(p)
    q = _clamp.activate(p, na, lin)
    assert all(o["status"] == 0 for o in lin)

    def compare(got, u_nom, lim, clamps, tag):
        cost, U = got
        on = 0
        for b, (co, Uo) in enumerate(_clamp.forward(p, lin, na, u_nom=u_nom, ctrl_lim=lim)):
            assert max(_rel(cost[b], co), _rel(U[b], Uo)) <= RTOL, (tag, b, _rel(cost[b], co), _rel(U[b], Uo))
            _check_limits(U[b], dict(U_alpha=Uo), lim, (tag, b))
            on += int(_clamp.on_limit(Uo, lim).sum())
        assert (on > 0) == clamps, (tag, on)

    _set_env(c, monkeypatch)
    with _engine(c, p) as e:
        st, _ = _backward(e, c, p, kp_ordered=_kp_ordered(c))
        assert np.all(st == 0)
        K, k = e.gains()
        for b, o in enumerate(lin):
            assert max(_rel(K[b], o["K"]), _rel(k[b], o["k"])) <= RTOL
        first = e.forward_linear(al, want_U=True)
        _check_dispatch(c, _launched(e), n_simd)
        compare(first, p["u_nom"], p["ctrl_lim"], False, "wide limits")
        e.upload_nominal(None, q["ctrl_lim"])
        compare(e.forward_linear(al, want_U=True), p["u_nom"], q["ctrl_lim"], True, "new limits")
        e.upload_nominal(q["u_nom"], None)
        compare(e.forward_linear(al, want_U=True), q["u_nom"], q["ctrl_lim"], True, "new nominal controls")
        e.upload_nominal(p["u_nom"], p["ctrl_lim"])
        again = e.forward_linear(al, want_U=True)
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])


@pytest.mark.parametrize("fused", [True, False])
def test_iterate_clamped_equals_staged(fused, monkeypatch):
    """kpilqr_iterate with the clamp active gives bit for bit what the staged calls give."""
    for key in S.ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    p0 = synth.make_problem(task="panda_reaching", T=50, batch=3, min_N=5)
    lin = _clamp.linearise(p0)
    p = _clamp.activate(p0, 6, lin)
    _clamp.assert_conditions(_clamp.conditions(p, 6, lin), 6, "panda")
    al = orc.alphas(6)
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=3, fused=fused) as e:
        assert ("fused" in e.forward_variant) == fused
        synth.upload(e, p)
        e.fd_difference()
        if not fused:
            e.interpolate()
            e.cost_derivs()
        st, dJ = e.backward(p["lam"], 100)
        K, k = e.gains()
        cost = e.forward_linear(al)
    for b, o in enumerate(_clamp.references(p, 6, lin)):
        assert st[b] == 0 and max(_rel(K[b], o["K"]), _rel(cost[b], o["cost_pred"])) <= RTOL
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=3, fused=fused) as e:
        synth.upload(e, p)
        e.iterate(p["lam"], 100, al)
        res = e.results()
        Ki, ki = e.gains()
    assert np.array_equal(res["cost_pred"], cost) and np.array_equal(res["delta_J"], dJ) and np.array_equal(res["status"], st)
    assert np.array_equal(Ki, K) and np.array_equal(ki, k)
