"""The factorisation path of the uniform one-wave backward sweep (fused_mfma.hip, kp_factor_path): the first step of a sweep, every
checked step and every re-seed leave the step's straight line for an out-of-line function that reads the step's LDS image and hands
the gains column, the seed of the running inverse and the PD verdict back in registers.  What can go wrong is in the hand-over:

  * the inverse that comes back seeds the refresh of the steps below (Xinv, Xprev, haveX): pd_stride 1 runs EVERY step through the
    function, 2 and 5 alternate it with the refresh across the key-point crossings (every 3 steps), 100 -- the bench's -- takes it on
    the first step only; the gains of stride 100 and of stride 1 of the same library agree to 1e-9;
  * the verdict: a checked step that is not PD ends the sweep with the oracle's status (negative running weights, the construction of
    tests/_lambda_retry.py: with pd_stride 5 the first check, at step T - 5, fails, and the unchecked indefinite steps above it go
    through the pivoted slow path, which stays with the caller; with pd_stride 1 the step below the terminal one fails);
  * every shape of the one-wave sweeps, (14,7) (12,3) (10,3) (4,1), with the constant residual Jacobian and with Jacobians per step,
    on the key-point ordered payload (`raw`) and on job lists (`kpc`);
  * 513 trajectories of (14,7) in the default environment: the library's own choice there is the one-wave sweep, not the wave pair.

T = 12, key-points every 3 steps, 3 trajectories.  K, k, delta_J and the predicted costs are held to oracle.pipeline.run_trajectory at
1e-9, the status exactly (the bar of tools/ab_check.py).  The oracle's runs are made once per problem and shared; the CPU test at
the bottom asserts on the oracle alone what the GPU tests rely on: success where success is asserted, and WHICH step fails."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import Engine, synth

gpu = pytest.mark.gpu

RTOL = 1e-9
ALPHAS = orc.alphas(6)
T, MIN_N, BATCH, BIG = 12, 3, 3, 513
SHAPES = {"panda_reaching": (14, 7), "hopper": (12, 3), "pentabot": (10, 3), "acrobot": (4, 1)}
PD_STRIDES = (1, 2, 5, 100)
WAVE_KEYS = ("KPILQR_FUSED_WAVES", "KPILQR_FUSED_FWD_WAVES", "KPILQR_FUSED_UNI", "KPILQR_FUSED_RAW")
# negative running weights w_run = -(|w_run| + 1) * FAIL_SCALE: pd_stride -> the status the sweep ends with, t + 1 of the failing
# step t (stride 5: the first check, t = T - 5; stride 1: t = T - 2, the first step under the running weights)
FAIL_SCALE = 20.0
FAIL_STATUS = {5: T - 5 + 1, 1: T - 2 + 1}


@functools.lru_cache(maxsize=None)
def problem(task, batch=BATCH):
    p = synth.make_problem(task=task, T=T, batch=batch, min_N=MIN_N)
    assert (p["n"], p["m"]) == SHAPES[task] and p["rx_const"] is not None
    return p


@functools.lru_cache(maxsize=None)
def failing_problem(task):
    p = synth.make_problem(task=task, T=T, batch=BATCH, min_N=MIN_N, dense_residuals=True)
    p["w_run"] = -(np.abs(p["w_run"]) + 1.0) * FAIL_SCALE
    return p


@functools.lru_cache(maxsize=None)
def reference(task, pd_stride, batch=BATCH):
    p = problem(task, batch)
    return [pipeline.run_trajectory(p, b, pd_stride=pd_stride) for b in range(batch)]


@functools.lru_cache(maxsize=None)
def failing_reference(task, pd_stride):
    p = failing_problem(task)
    return [pipeline.run_trajectory(p, b, pd_stride=pd_stride)["status"] for b in range(BATCH)]


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


@functools.lru_cache(maxsize=None)
def run(task, payload, rx_const, pd_stride, batch=BATCH, one_wave=True):
    """One kpilqr_iterate on a fresh context (the environment is read when it is created)."""
    p = problem(task, batch)
    saved = {k: os.environ.pop(k, None) for k in WAVE_KEYS}
    if one_wave:
        os.environ["KPILQR_FUSED_WAVES"] = os.environ["KPILQR_FUSED_FWD_WAVES"] = "1"
    try:
        e = Engine(p["dof"], p["m"], T, p["nr"], batch=batch, fused=True)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    with e:
        synth.upload(e, p, kp_ordered=(payload == "raw"), rx_const=rx_const)
        e.iterate(p["lam"], pd_stride, ALPHAS)
        res = e.results()
        K, k = e.gains()
        return dict(K=K, k=k, launch=e.last_launch("backward"), **res)


def assert_form(got, payload, rx_const):
    lb = got["launch"]
    assert ":w1:" in lb and ":uni" in lb and f":{payload}:" in lb and (":rxc" in lb) == rx_const, lb


def figures(got, want, b):
    return dict(K=relerr(got["K"][b], want["K"]), k=relerr(got["k"][b], want["k"]),
                delta_J=abs(float(got["delta_J"][b]) - float(want["delta_J"])) / abs(float(want["delta_J"])),
                cost_pred=relerr(got["cost_pred"][b], want["cost_pred"]))


def assert_oracle(got, refs, label, quiet=False):
    worst = dict(K=0.0, k=0.0, delta_J=0.0, cost_pred=0.0)
    for b, o in enumerate(refs):
        fig = figures(got, o, b)
        worst = {n: max(worst[n], v) for n, v in fig.items()}
        if not quiet:
            print(f"{label} b={b}: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
        assert got["status"][b] == o["status"] == 0, (label, b, got["status"][b], o["status"])
        assert all(v < RTOL for v in fig.values()), (label, b, fig)
    return worst


@gpu
@pytest.mark.parametrize("pd_stride", PD_STRIDES)
@pytest.mark.parametrize("rx_const", [True, False], ids=["rxc", "per_step"])
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("task", sorted(SHAPES))
def test_factor_path_against_the_oracle(task, payload, rx_const, pd_stride):
    got = run(task, payload, rx_const, pd_stride)
    assert_form(got, payload, rx_const)
    assert_oracle(got, reference(task, pd_stride), f"{task} {payload} {'rxc' if rx_const else 'per_step'} pd_stride {pd_stride}")


@gpu
@pytest.mark.parametrize("rx_const", [True, False], ids=["rxc", "per_step"])
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("task", sorted(SHAPES))
def test_refreshed_sweep_against_the_factorised_sweep(task, payload, rx_const):
    """stride 100 carries the inverse of the first step's call through every refresh; stride 1 takes a fresh one from the call at
    every step"""
    far, every = run(task, payload, rx_const, 100), run(task, payload, rx_const, 1)
    fig = dict(K=relerr(far["K"], every["K"]), k=relerr(far["k"], every["k"]), delta_J=relerr(far["delta_J"], every["delta_J"]))
    print(f"{task} {payload} {'rxc' if rx_const else 'per_step'} stride 100 vs 1: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    assert np.array_equal(far["status"], every["status"]) and not np.any(far["status"])
    assert all(v < RTOL for v in fig.values()), fig


@gpu
@pytest.mark.parametrize("pd_stride", sorted(FAIL_STATUS))
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("task", sorted(SHAPES))
def test_failing_check_ends_the_sweep_where_the_oracle_ends_it(task, payload, pd_stride, monkeypatch):
    for key in WAVE_KEYS:
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("KPILQR_FUSED_WAVES", "1")
    monkeypatch.setenv("KPILQR_FUSED_FWD_WAVES", "1")
    p = failing_problem(task)
    with Engine(p["dof"], p["m"], T, p["nr"], batch=BATCH, fused=True) as e:
        synth.upload(e, p, kp_ordered=(payload == "raw"))
        st, _ = e.backward(p["lam"], pd_stride=pd_stride)
        lb = e.last_launch("backward")
    assert ":w1:" in lb and ":uni" in lb and f":{payload}:" in lb, lb
    want = failing_reference(task, pd_stride)
    print(f"{task} {payload} pd_stride {pd_stride}: status {list(st)} oracle {want}")
    assert list(st) == want == [FAIL_STATUS[pd_stride]] * BATCH


@gpu
def test_default_dispatch_above_512_trajectories_is_the_one_wave_sweep():
    got = run("panda_reaching", "raw", True, 100, batch=BIG, one_wave=False)
    assert_form(got, "raw", True)
    assert ":pairh" not in got["launch"], got["launch"]
    worst = assert_oracle(got, reference("panda_reaching", 100, BIG), f"batch {BIG}", quiet=True)
    print(f"batch {BIG}, {got['launch']}: worst " + " ".join(f"{n} {v:.2e}" for n, v in worst.items()))


def test_oracle_outcomes_the_gpu_tests_rely_on():
    """(CPU) status 0 on every problem on which success is asserted; under the negative weights the sweep fails at the step named in
    FAIL_STATUS, and with stride 5 the unchecked steps above it are indefinite too (stride 1 fails there): the pivoted path runs"""
    for task in SHAPES:
        for pd_stride in PD_STRIDES:
            assert all(o["status"] == 0 for o in reference(task, pd_stride)), (task, pd_stride)
        for pd_stride, status in FAIL_STATUS.items():
            assert failing_reference(task, pd_stride) == [status] * BATCH, (task, pd_stride, failing_reference(task, pd_stride))
    assert FAIL_STATUS[1] > FAIL_STATUS[5]
