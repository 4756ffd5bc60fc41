"""Every sweep family against the CPU oracle at the shortest horizons: the cases of tests/_horizons.py (T = 2 .. 9 on every
form, 4 .. 13 on the six-set general forward, the block edges 15 and 16, key-points on every and every second step), each run as
tests/test_gpu_shapes.py runs its cases -- through the C ABI, with the variant and wave form asserted -- and compared with
oracle.pipeline.run_trajectory; and a PD failure pinned to a chosen step of a short horizon, checked at every step."""
import pytest

import _horizons as HZ
import _shapes as S
from _shape_run import RTOL, _backward, _check, _check_dispatch, _engine, _n_simd, _problem, _rel, _run, _set_env
from oracle import pipeline

pytestmark = pytest.mark.gpu

_CASES = HZ.cases()
_FAIL = HZ.failure_cases()


@pytest.mark.parametrize("c", _CASES, ids=[HZ.case_id(c) for c in _CASES])
def test_horizon_matches_oracle(c, monkeypatch):
    n_simd = _n_simd()
    p = _problem(c, min_N=c["min_N"])
    g = _run(c, p, monkeypatch, kp_ordered=c["kp_ordered"])
    _check_dispatch(c, g, n_simd)
    assert g["variants"][0] == c["variant"], g["variants"]
    refs = [pipeline.run_trajectory(p, b, n_alpha=c["n_alpha"], want_U=True) for b in range(p["batch"])]
    assert all(o["status"] == 0 for o in refs)
    _check(g, refs, range(p["batch"]), HZ.case_id(c))


@pytest.mark.parametrize("c", _FAIL, ids=[HZ.failure_id(c) for c in _FAIL])
def test_failure_position(c, monkeypatch):
    """Trajectory 1 fails the PD test (made on every step: pd_stride = 1) at step t* and nowhere else: the status is t* + 1 whatever
    the place of t* in a pair of steps, at the terminal step and at step 0, and trajectory 0, beside it in the batch, is
    untouched.  (K of the failed trajectory is undefined, include/kpilqr.h.)"""
    p = HZ.failing_problem(_problem(c), c["t_star"])
    refs = [pipeline.run_trajectory(p, b, pd_stride=1, stages=("fd", "interp", "cost", "bwd")) for b in range(2)]
    assert [o["status"] for o in refs] == [0, c["t_star"] + 1]
    _set_env(c, monkeypatch)
    with _engine(c, p) as e:
        st, dJ = _backward(e, c, p, c["kp_ordered"], pd=1)
        K, k = e.gains()
        variant, launch = e.backward_variant, e.last_launch("backward")
    d = S.dispatch(c["dof"], c["m"], c["nr"], c["T"], c["n_alpha"], c["batch"], _n_simd(), c["flags"], c["env"], False, False, True)
    assert variant == c["variant"] == d["variants"][0], (variant, d["variants"])
    want = d["launch"][0]
    assert launch.startswith(want) if ":" not in want else want in launch + ":", (launch, want)
    print(HZ.failure_id(c), "status", list(st))
    assert list(st) == [0, c["t_star"] + 1], (HZ.failure_id(c), list(st))
    o = refs[0]
    errs = dict(K=_rel(K[0], o["K"]), k=_rel(k[0], o["k"]), delta_J=abs(dJ[0] - o["delta_J"]) / max(abs(o["delta_J"]), 1e-300))
    print(HZ.failure_id(c), errs)
    assert max(errs.values()) <= RTOL, (HZ.failure_id(c), launch, errs)
