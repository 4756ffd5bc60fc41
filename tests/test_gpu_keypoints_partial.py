"""GPU tests of key-point placement on the device for a listed subset of the batch: kpilqr_upload_states_partial puts the listed
trajectories' states in place, kpilqr_generate_keypoints_partial places their lists (csrc/keypoints.hip, the LISTED instantiation
of k_kp_flags and k_kp_fill over compact rows) and leaves the context as kpilqr_update_keypoints with those lists would -- a
by-entry payload of the other trajectories carried over, the listed ranges pending --, kpilqr_get_keypoints_partial reads the new
lists back compact.

Lists are compared with the oracle's kp_* functions exactly (the decisions are bit for bit the oracle's); results behind a carried
payload bit for bit with a twin context that was given the same lists through kpilqr_update_keypoints (both run the same tail and
the same kernels) and with the oracle at the suite's 1e-9.  The cases and what makes them meaningful: tests/_keypoints_partial.py,
tests/test_keypoints_partial_inputs.py."""
import numpy as np
import pytest

import _keypoints_partial as C
import _sequences as Q
from oracle import oracle as orc, pipeline
from test_gpu_partial_regeneration import _payload, _problem, _raises, _rest
from trajoptkp_amd import Engine
from trajoptkp_amd.engine import _ptr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -5
ALPHAS = orc.alphas(6)


def _engine(c, **kw):
    dof = c["dof"]
    return Engine(dof, min(dof, 7), c["T"], 3, batch=c["batch"], generic=(2 * dof + 2 > 64), **kw)


def _place_whole(e, c):
    if c["method"] != "set_interval":             # (set_interval reads no states: those cases run without any)
        e.upload_states(c["X0"])
    e.generate_keypoints(*c["args0"])


def _place_listed(e, c, traj):
    if c["method"] != "set_interval":
        e.upload_states_partial(traj, c["X1"][traj])
    e.generate_keypoints_partial(traj, *c["args1"])


def _size_query(e, traj):
    tr = np.ascontiguousarray(traj, np.int32)
    offs = np.zeros(len(tr) * e.dof + 1, np.int32)
    return e._L.kpilqr_get_keypoints_partial(e._h, len(tr), _ptr(tr), _ptr(offs), None, 0), offs


def _check_lists(e, c, traj):
    """The merged lists for everybody, the listed part compact, the size query."""
    wo, wt = C.csr(C.merged(c["lists0"], c["lists1"], traj))
    o, t = e.get_keypoints()
    assert np.array_equal(o, wo) and np.array_equal(t, wt), "merged lists"
    lo, lt = C.csr([c["lists1"][b] for b in traj])
    po, pt = e.get_keypoints_partial(traj)
    assert np.array_equal(po, lo) and np.array_equal(pt, lt), "the listed trajectories' lists, compact"
    total, qo = _size_query(e, traj)
    assert total == len(lt) and np.array_equal(qo, lo), "size query"


# ---- 1. the lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.SUBSETS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("method", C.METHODS)
def test_listed_placement_matches_the_oracle(method, shape, name):
    c = C.list_case(method, shape)
    traj = C.subset(name, c["batch"])
    with _engine(c) as e:
        _place_whole(e, c)
        _place_listed(e, c, traj)
        _check_lists(e, c, traj)
        # the lists of any subset, device-placed or not, come back compact
        other = [b for b in range(c["batch"]) if b not in traj][:2] + traj[-1:]
        other = sorted(set(other))
        po, pt = e.get_keypoints_partial(other)
        lo, lt = C.csr([C.merged(c["lists0"], c["lists1"], traj)[b] for b in other])
        assert np.array_equal(po, lo) and np.array_equal(pt, lt)
        if method != "set_interval":
            # the states went to the listed trajectories' rows and to nobody else's: a whole placement now sees X1 there, X0 elsewhere
            e.generate_keypoints(*c["args0"])
            o, t = e.get_keypoints()
            wo, wt = C.csr(C.merged(c["lists0"], c["lists1"], traj))
            assert np.array_equal(o, wo) and np.array_equal(t, wt), "states of the subset"


def test_more_than_one_block_of_listed_lists():
    c = C.many_case()
    traj = C.many_subset()
    with _engine(c) as e:
        _place_whole(e, c)
        _place_listed(e, c, traj)
        _check_lists(e, c, traj)


# ---- 2. a by-entry payload carried across the placement ---------------------------------------------------------------------------
def _carry_problems():
    c = C.carry_case()
    dof, T = c["dof"], c["T"]
    p0 = _problem(c["task"], T, [C.rows_of(l, dof, T) for l in c["lists0"]])
    p1 = _problem(c["task"], T, [C.rows_of(l, dof, T) for l in C.merged(c["lists0"], c["lists1"], c["traj"])])
    return c, p0, p1


def _fused(p):
    e = Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=True)
    assert "fused" in e.backward_variant
    return e


def _observe(e, p):
    e.iterate(p["lam"], 100, ALPHAS)
    res = e.results()
    K, k = e.gains()
    return dict(K=K, k=k, delta_J=res["delta_J"], cost=res["cost_pred"], status=res["status"],
                launch=(e.last_launch("backward"), e.last_launch("forward"), e.last_launch("linearise")))


def _bit_equal(got, want, what):
    assert got["launch"] == want["launch"], (what, got["launch"], want["launch"])
    for key in ("status", "K", "k", "delta_J", "cost"):
        assert np.array_equal(got[key], want[key]), (what, key)


def _oracle_check(got, p):
    for b in range(p["batch"]):
        o = pipeline.run_trajectory(p, b)
        assert o["status"] == 0 and got["status"][b] == 0
        errs = dict(K=Q._rel(got["K"][b], o["K"]), k=Q._rel(got["k"][b], o["k"]), cost=Q._rel(got["cost"][b], o["cost_pred"]),
                    delta_J=abs(got["delta_J"][b] - o["delta_J"]) / max(abs(o["delta_J"]), 1e-300))
        assert max(errs.values()) <= Q.RTOL, (b, errs)


def _start(e, c, p0, form):
    """A whole linearisation on device-placed lists, and one iteration."""
    e.upload_states(c["X0"])
    e.generate_keypoints(*c["args0"])
    _payload(e, p0, form)
    _rest(e, p0)
    return _observe(e, p0)


@pytest.mark.parametrize("form", ["fd_kp", "cols"])
def test_payload_is_carried_as_by_update_keypoints(form):
    c, p0, p1 = _carry_problems()
    traj = c["traj"]
    lo, lt = C.csr([c["lists1"][b] for b in traj])
    with _fused(p0) as e:
        first = _start(e, c, p0, form)
        e.upload_states_partial(traj, c["X1"][traj])
        e.generate_keypoints_partial(traj, *c["args1"])
        po, pt = e.get_keypoints_partial(traj)            # (what the host FD loop fills the listed records by)
        assert np.array_equal(po, lo) and np.array_equal(pt, lt)
        _payload(e, p1, form, traj)
        _rest(e, p1)
        got = _observe(e, p1)
    with _fused(p0) as e:                                 # the twin: the same lists through kpilqr_update_keypoints
        _bit_equal(_start(e, c, p0, form), first, "before the update")
        e.update_keypoints(traj, lo, lt)
        _payload(e, p1, form, traj)
        _rest(e, p1)
        want = _observe(e, p1)
    _bit_equal(got, want, "twin through kpilqr_update_keypoints")
    _oracle_check(got, p1)
    assert not np.array_equal(got["K"][traj], first["K"][traj])


# ---- 3. the pending state -----------------------------------------------------------------------------------------------------------
def test_pending_ranges_between_the_placement_and_the_partial_upload():
    c, p0, p1 = _carry_problems()
    traj = c["traj"]
    lo, lt = C.csr([c["lists1"][b] for b in traj])
    with _fused(p0) as e:
        _start(e, c, p0, "fd_kp")
        e.upload_states_partial(traj, c["X1"][traj])
        e.generate_keypoints_partial(traj, *c["args1"])
        _rest(e, p1)
        for call in (lambda: e.backward(p1["lam"]), lambda: e.iterate(p1["lam"], 100, ALPHAS),
                     lambda: e.generate_keypoints_partial([0], *c["args1"]), lambda: e.update_keypoints(traj, lo, lt)):
            msg = _raises(ERR_STATE, call)
            assert "pending" in msg and "partial" in msg, msg
        po, pt = e.get_keypoints_partial(traj)            # reads lists, not payload
        assert np.array_equal(po, lo) and np.array_equal(pt, lt)
        _check_lists(e, c, traj)
        _payload(e, p1, "fd_kp")                          # a whole payload clears the pending state
        got = _observe(e, p1)
        e.generate_keypoints_partial([0], "set_interval", 4)      # ... and the next placement is taken again
    with _fused(p1) as e:
        e.set_keypoints_rows(p1["kp_rows"])
        _payload(e, p1, "fd_kp")
        _rest(e, p1)
        want = _observe(e, p1)
    if got["launch"] == want["launch"]:
        _bit_equal(got, want, "after a whole upload")
    else:
        assert max(Q._rel(got[k], want[k]) for k in ("K", "k", "delta_J", "cost")) <= Q.RTOL_FORMS


# ---- 4. refusals that change nothing ------------------------------------------------------------------------------------------------
def _snapshot(e, p):
    o, t = e.get_keypoints()
    status, dJ = e.backward(p["lam"])
    K, k = e.gains()
    return o, t, status, dJ, K, k


def _unchanged(e, p, before, what):
    for a, b in zip(_snapshot(e, p), before):
        assert np.array_equal(a, b), what


def test_refusals_change_nothing():
    c, p0, p1 = _carry_problems()
    dof, T, B = c["dof"], c["T"], c["batch"]
    thr = c["args1"][3]
    X1 = c["X1"]
    with _fused(p0) as e:
        _raises(ERR_STATE, e.generate_keypoints_partial, [0], "set_interval", 3)             # before any key-points exist
        e.set_keypoints_rows(p0["kp_rows"])               # lists from the host: nobody's states were ever uploaded
        _payload(e, p0, "fd_kp")
        _rest(e, p0)
        e.iterate(p0["lam"], 100, ALPHAS)
        before = _snapshot(e, p0)
        for traj in ([2, 1], [1, 1], [-1, 0], [0, B]):    # strictly increasing, within [0, batch)
            _raises(ERR_ARG, e.upload_states_partial, traj, X1[:2])
            _raises(ERR_ARG, e.generate_keypoints_partial, traj, *c["args1"])
            _raises(ERR_ARG, e.get_keypoints_partial, traj)
        _unchanged(e, p0, before, "bad lists")
        msg = _raises(ERR_ARG, e.generate_keypoints_partial, [1], "iterative_error", 2, 20, thr, C.DT)
        assert "iterative_error" in msg
        _raises(ERR_ARG, e.generate_keypoints_partial, [1], "velocity_change", 0, 20, thr, C.DT)
        _raises(ERR_ARG, e.generate_keypoints_partial, [1], "adaptive_jerk", 2, 20, thr, 0.0)
        _raises(ERR_ARG, e.generate_keypoints_partial, [1], "velocity_change", 2, 20, None, C.DT)
        _unchanged(e, p0, before, "bad placement arguments")
        msg = _raises(ERR_STATE, e.generate_keypoints_partial, [1, 2], *c["args1"])
        assert "trajectory 1 " in msg, msg
        e.upload_states_partial([1], X1[[1]])
        msg = _raises(ERR_STATE, e.generate_keypoints_partial, [1, 2], *c["args1"])
        assert "trajectory 2 " in msg, msg
        _unchanged(e, p0, before, "a listed trajectory without states")
        # too small a capacity; count = 0
        tr = np.array([1, 2], np.int32)
        offs, times = np.zeros(2 * dof + 1, np.int32), np.zeros(4, np.int32)
        assert e._L.kpilqr_get_keypoints_partial(e._h, 2, _ptr(tr), _ptr(offs), _ptr(times), 4) == ERR_ARG
        e.upload_states_partial([], np.zeros((0, T, 2 * dof)))
        e.generate_keypoints_partial([], *c["args1"])
        po, pt = e.get_keypoints_partial([])
        assert list(po) == [0] and len(pt) == 0
        _unchanged(e, p0, before, "count = 0")
        # a trajectory whose states were given is placed; set_interval needs nobody's
        e.generate_keypoints_partial([1], *c["args1"])
        po, pt = e.get_keypoints_partial([1])
        lo, lt = C.csr([c["lists1"][1]])
        assert np.array_equal(po, lo) and np.array_equal(pt, lt)
    with _fused(p0) as e:
        e.set_keypoints_rows(p0["kp_rows"])
        e.generate_keypoints_partial([0, 3], "set_interval", 4)                              # without any states
        o, t = e.get_keypoints()
        every4 = [np.unique(np.r_[np.arange(0, T, 4), T - 1])] * dof
        wo, wt = C.csr([every4 if b in (0, 3) else c["lists0"][b] for b in range(B)])
        assert np.array_equal(o, wo) and np.array_equal(t, wt)
        # a whole upload of states sets everybody's byte, a resize clears them
        e.upload_states(c["X0"])
        e.generate_keypoints_partial([2], *c["args1"][:3], thr, C.DT)
        e.resize(dof, p0["m"], T)
        e.set_keypoints_rows(p0["kp_rows"])
        msg = _raises(ERR_STATE, e.generate_keypoints_partial, [2], *c["args1"])
        assert "trajectory 2 " in msg, msg


# ---- 5. one long-lived context through a scripted mix -------------------------------------------------------------------------------
class PlacedShadow(Q.Shadow):
    """tests/_sequences.py's shadow with one more op: new lists for a subset placed on the device from new states of that subset."""

    def illegal(self, op):
        if op["op"] == "generate_keypoints_partial":
            if self.rows is None:
                return "no key-points yet"
            return "ranges are pending" if self.pending else None
        return super().illegal(op)

    def _op_generate_keypoints_partial(self, op, rng, e):
        dof, _, T, _ = self.dims
        traj = list(op["traj"])
        X = np.stack([Q._kp_states(rng, dof, T) for _ in traj])
        thr = rng.uniform(0.5, 20.0, dof)
        lists = [C.dof_lists(orc.kp_velocity_change(dof, T, 2, 12, thr, Xb), dof, T) for Xb in X]
        self.rows = list(self.rows)
        for b, l in zip(traj, lists):
            self.rows[b] = C.rows_of(l, dof, T)
        self._keypoints_replaced(traj, update=True)
        if e:
            e.upload_states_partial(traj, X)
            e.generate_keypoints_partial(traj, "velocity_change", 2, 12, thr, 0.01)
            po, pt = e.get_keypoints_partial(traj)
            lo, lt = C.csr(lists)
            assert np.array_equal(po, lo) and np.array_equal(pt, lt), "kpilqr_get_keypoints_partial differs from the shadow's lists"


MIX = [
    dict(op="generate_keypoints", method="velocity_change", seed=1),                         # 1. whole placement
    dict(op="upload_payload", kind="fd_kp", seed=2),                                         # 2. payload (and the rest of a first linearisation)
    dict(op="upload_residuals", what="r+rx", seed=3), dict(op="weights", seed=4), dict(op="nominal", seed=5),
    dict(op="observe", how="iterate", gains="all", seed=6),                                  # 3.
    dict(op="generate_keypoints_partial", traj=[1, 2], seed=7),                              # 4. partial placement
    dict(op="upload_payload_partial", seed=8),                                               # 5.
    dict(op="observe", how="iterate", gains="all", seed=9),                                  # 6.
    dict(op="update_keypoints", subset="pair", seed=10),                                     # 7. kpilqr_update_keypoints from the host
    dict(op="upload_payload_partial", seed=11),                                              # 8.
    dict(op="stage", call="get_keypoints"),
    dict(op="generate_keypoints_partial", traj=[0, 3], seed=12),                             # 9. partial placement of another list
    dict(op="stage", call="get_keypoints"),
    dict(op="upload_payload", kind="cols", seed=13, same_kp=False),                          # 10. a whole payload
    dict(op="observe", how="staged", gains="subset", subset=[0, 3], seed=14),                # 11.
    dict(op="generate_keypoints_partial", traj=[3], seed=15),                                # ... and once more on the column payload
    dict(op="upload_payload_partial", seed=16),
    dict(op="observe", how="iterate", gains="all", seed=17),
]


@pytest.mark.parametrize("kind", ["fused", "fused_union", "records_t1"])
def test_scripted_mix_on_one_context(kind, monkeypatch):
    sh = PlacedShadow(kind)
    n_obs = 0
    with Q.make_engine(sh, monkeypatch.setenv, monkeypatch.delenv) as e:
        for i, op in enumerate(MIX):
            got = sh.apply(op, e)
            if op["op"] != "observe":
                continue
            errs = Q.oracle_errors(got, sh.oracle())
            assert max(errs.values()) <= Q.RTOL, (i, op, "oracle", got["launch"], errs)
            same, diff = Q.fresh_errors(got, Q.fresh_observation(sh, op, monkeypatch.setenv, monkeypatch.delenv))
            assert diff <= Q.RTOL_FORMS, (i, op, "fresh context", got["launch"], diff)
            print(f"mix {kind} op {i}: launch {got['launch'][0]}, fresh context {'bit-equal' if same else f'{diff:.1e}'}, oracle {max(errs.values()):.1e}")
            n_obs += 1
    assert n_obs == 4
