"""Every compiled kernel instantiation against the CPU oracle, at problems of any shape (synth.shape_task), not only the task
table's: the cases of tests/_shapes.py (the dispatch restated, with the smallest and largest shape of every key), each run
through the C ABI -- FD, interpolation, cost, backward, forward over the alphas -- and compared with
oracle.pipeline.run_trajectory.  Each case also asserts the variant (and, for the fused sweeps, the wave form) the table
predicts, so that a shape that silently falls back does not count as covering a kernel."""
import pytest

import _shapes as S
from _shape_run import _case_id, _check, _check_dispatch, _n_simd, _problem, _run, _take
from oracle import pipeline
from trajoptkp_amd import Engine, synth
from trajoptkp_amd.engine import KpilqrError

pytestmark = pytest.mark.gpu

_CASES = [c for c in S.cases(1024) if c["why"] != "refused"]


@pytest.mark.parametrize("c", _CASES, ids=[_case_id(c) for c in _CASES])
def test_shape_matches_oracle(c, monkeypatch):
    n_simd = _n_simd()
    p = _problem(c)
    kp_ordered = bool(c["flags"] & S.FLAG_FUSED) and (c["dof"] + c["nr"]) % 2 == 1     # both payload forms over the fused cases
    g = _run(c, p, monkeypatch, kp_ordered=kp_ordered)
    _check_dispatch(c, g, n_simd)
    refs = [pipeline.run_trajectory(p, b, n_alpha=c["n_alpha"], want_U=True) for b in range(p["batch"])]
    assert all(o["status"] == 0 for o in refs) or c["why"] == "long"
    _check(g, refs, range(p["batch"]), _case_id(c), p=p, n_alpha=c["n_alpha"])


def test_batch_boundaries(monkeypatch):
    """n_simd and n_simd + 1 trajectories (excl / plain kernels of the one-tile and one-wave fused sweeps), n_simd / 4 and one more
    (the tiled state / cost forward): 7 distinct trajectories tiled, every one of the batch checked against its oracle."""
    n_simd = _n_simd()
    for c in S.batch_cases(n_simd):
        c = dict(c, T=17)
        base = _problem(c, batch=7, config_id=5)
        refs = [pipeline.run_trajectory(base, b, n_alpha=c["n_alpha"], want_U=True) for b in range(7)]
        p = _take(synth.tile_problem(base, -(-c["batch"] // 7)), c["batch"])
        g = _run(c, p, monkeypatch, kp_ordered=bool(c["flags"] & S.FLAG_FUSED))
        _check_dispatch(c, g, n_simd)
        _check(g, refs, range(c["batch"]), _case_id(c), p=base, n_alpha=c["n_alpha"])


def test_generic_lds_limit_refused_at_create(monkeypatch):
    """The largest state the generic backward sweep takes with 7 controls runs (test_shape_matches_oracle, dof 46); the next is
    refused by kpilqr_create with KPILQR_ERR_ARG."""
    for key in S.ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    dof = S.GENERIC_MAX_DOF_M7 + 1
    with pytest.raises(KpilqrError) as ei:
        Engine(dof, 7, 5, 4, batch=2)
    assert ei.value.code == -1 and "LDS" in str(ei.value)
