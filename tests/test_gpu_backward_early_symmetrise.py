"""The uniform one-wave backward sweeps (fused_mfma.hip, `ESYM`): the Qzz tile goes through LDS right behind its product, in front of
the refresh -- at (14,7) the merged halved tile, Qs = Qm/2 + (Qm/2)', at (4,1), (12,3), (10,3) Qs = (Qzz + Qzz')/2 -- and
V = Qs + K'G with G = Quz - lambda K in full leaves the last product of the step as it is: no transposition behind it.  The terminal
step (V = Lzz), the factorised and the slow path keep their statements; the wave pairs and the general form keep the transposition
behind the product (the general form is the reference of the last test).

The shapes are the smallest at which this can go wrong: T = 2 is the terminal step and the first Qs; key-points every 1, 2 and 5 steps
make every step a peeled one, peeled and inner steps alternate, and T = 11 has the headline's segment of four inner steps; lambda at
both ends of the reference's range; pd_stride 2 and 3 put the LDS images of the factorisation and the early image in KP_LDS_V into one
step, followed by refreshed steps; dense residuals have r_u != 0 (Luz rides in D1, l_uu in D2).  The gated twin runs under a lambda
retry schedule whose first lambda fails on the oracle for some trajectories; the listed twin sweeps 5 of 16 trajectories.  Acrobot,
hopper and pentabot (one live register) run T = 11 with key-points every 5 steps, with and without a PD check every 3 steps.
(T = 1, the terminal step alone, is not a sweep the library runs: kpilqr_create refuses T < 2, tests/test_abi.py.)

Everything is held to oracle.pipeline.run_trajectory at 1e-9 (K, k, delta_J, predicted costs; status exactly), forms of one sweep to
each other at 1e-12.  The oracle's runs are made once per problem and shared; the CPU test at the bottom asserts that every input on
which success is asserted succeeds on the oracle, and that the retry problem has both outcomes."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import Engine, synth

import _lambda_retry as lr

gpu = pytest.mark.gpu

RTOL = 1e-9          # to the oracle
FTOL = 1e-12         # between forms of the same sweep
ALPHAS = orc.alphas(6)
BATCH = 3
HORIZONS = (2, 3, 11)
INTERVALS = (1, 2, 5)                                        # key-points every min_N steps
LEGS = {"rxc": (False, True), "per_step": (False, False), "dense": (True, False)}          # dense residuals, constant-Jacobian upload
LAMBDAS = (1e-4, 10.0)
PD_LOW = (2, 3)
SMALL = ("acrobot", "hopper", "pentabot")                    # (4,1), (12,3), (10,3): NCU = 1, Qzz whole
# the gated twin: the recipe of tests/test_gpu_backward_inner_step.py (Panda T = 11 under negative running weights, a PD check every
# RETRY_PD steps; the constant-Jacobian leg fails at lambda 1e-4 and settles from 0.1 on, the dense leg fails at 0.1 and settles from 1 on)
RETRY_PD, RETRY_BATCH = 3, 4
RETRY = {"rxc": (20.0, (1e-4, 0.1, 1e-4, 1.0)), "dense": (3.0, (0.1, 1.0, 10.0, 0.1))}          # leg: scale, start lambdas
LISTED_BATCH, LISTED = 16, [1, 6, 7, 12, 15]                 # the listed twin: a scattered subset


@functools.lru_cache(maxsize=None)
def problem(T, min_N, dense, batch=BATCH, lam=0.1, task="panda_reaching"):
    return synth.make_problem(task=task, T=T, batch=batch, min_N=min_N, one_sided_frac=0.25, dense_residuals=dense, lam=lam)


@functools.lru_cache(maxsize=None)
def reference(T, min_N, dense, pd_stride=100, batch=BATCH, lam=0.1, task="panda_reaching"):
    p = problem(T, min_N, dense, batch, lam, task)
    return [pipeline.run_trajectory(p, b, pd_stride=pd_stride) for b in range(p["batch"])]


@functools.lru_cache(maxsize=None)
def retry_problem(leg):
    scale, lam0 = RETRY[leg]
    p = dict(synth.make_problem(task="panda_reaching", T=11, batch=RETRY_BATCH, min_N=5, dense_residuals=LEGS[leg][0]))
    p["w_run"] = -(np.abs(p["w_run"]) + 1.0) * scale
    p["lam0"] = np.array(lam0)
    return p


@functools.lru_cache(maxsize=None)
def retry_reference(leg):
    """tests/_lambda_retry.py's reference loop with the default schedule (factor 10, max_lambda 10, 6 attempts) on retry_problem()"""
    p = retry_problem(leg)
    out = []
    for b in range(p["batch"]):
        lam, seen = float(p["lam0"][b]), []
        while True:
            o = pipeline.run_trajectory(p, b, lam=lam, pd_stride=RETRY_PD)
            seen.append(lam)
            nxt, ex = lr.next_lambda(lam, lr.FACTOR, lr.MAX_LAMBDA)
            if o["status"] == 0 or ex or len(seen) >= lr.MAX_ATTEMPTS:
                break
            lam = nxt
        out.append(dict(out=o, visited=tuple(seen), lam=lam))
    return out


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


@pytest.fixture(autouse=True)
def one_wave(monkeypatch):
    monkeypatch.delenv("KPILQR_FUSED_UNI", raising=False)
    monkeypatch.setenv("KPILQR_FUSED_WAVES", "1")
    monkeypatch.setenv("KPILQR_FUSED_FWD_WAVES", "1")


def fresh_engine(p, general=False):
    """(the environment is read when the context is created)"""
    if general:
        os.environ["KPILQR_FUSED_UNI"] = "0"
    try:
        return Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=True)
    finally:
        os.environ.pop("KPILQR_FUSED_UNI", None)


@functools.lru_cache(maxsize=None)
def run(T, min_N, dense, payload, rx_const, pd_stride=100, general=False, lam=0.1, task="panda_reaching"):
    """One kpilqr_iterate of the problem on a fresh context."""
    p = problem(T, min_N, dense, lam=lam, task=task)
    with fresh_engine(p, general) as e:
        synth.upload(e, p, kp_ordered=(payload == "raw"), rx_const=rx_const)
        e.iterate(p["lam"], pd_stride, ALPHAS)
        res = e.results()
        K, k = e.gains()
        return dict(K=K, k=k, launch=e.last_launch("backward"), **res)


def assert_form(got, payload, rxc=None, general=False):
    lb = got["launch"]
    assert ":w1:" in lb and f":{payload}:" in lb, lb
    assert (":uni" in lb) == (not general), lb
    if rxc is not None:
        assert (":rxc" in lb) == rxc, lb


def figures(got, want, b=None):
    sl = slice(None) if b is None else b
    return dict(K=relerr(got["K"][sl], want["K"]), k=relerr(got["k"][sl], want["k"]),
                delta_J=abs(float(got["delta_J"][sl]) - float(want["delta_J"])) / abs(float(want["delta_J"])) if b is not None
                else relerr(got["delta_J"], want["delta_J"]),
                cost_pred=relerr(got["cost_pred"][sl], want["cost_pred"]))


def assert_oracle(got, refs, label):
    for b, o in enumerate(refs):
        fig = figures(got, o, b)
        print(f"{label} b={b}: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
        assert got["status"][b] == o["status"] == 0, (label, b, got["status"][b], o["status"])
        assert all(v < RTOL for v in fig.values()), (label, b, fig)


# ---- 1. Panda (14,7) at small horizons: every interval, payload and Jacobian leg --------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("min_N", INTERVALS)
@pytest.mark.parametrize("T", HORIZONS)
def test_panda_sweep_against_the_oracle(T, min_N, payload, leg):
    dense, rx_const = LEGS[leg]
    got = run(T, min_N, dense, payload, rx_const)
    assert_form(got, payload, rxc=rx_const)
    assert_oracle(got, reference(T, min_N, dense), f"T={T} every {min_N} {payload} {leg}")


@gpu
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("min_N", INTERVALS)
@pytest.mark.parametrize("T", HORIZONS)
def test_constant_jacobian_leg_against_the_per_step_leg(T, min_N, payload):
    rxc, per = run(T, min_N, False, payload, True), run(T, min_N, False, payload, False)
    assert_form(rxc, payload, rxc=True); assert_form(per, payload, rxc=False)
    fig = figures(rxc, per)
    print(f"T={T} every {min_N} {payload} rxc vs per-step: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    assert np.array_equal(rxc["status"], per["status"])
    assert all(v < FTOL for v in fig.values()), fig


# ---- 2. lambda at both ends of the reference's range ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("lam", LAMBDAS)
def test_lambda_at_both_ends(lam, leg):
    dense, rx_const = LEGS[leg]
    got = run(11, 5, dense, "raw", rx_const, lam=lam)
    assert_form(got, "raw", rxc=rx_const)
    assert_oracle(got, reference(11, 5, dense, lam=lam), f"lambda {lam:g} {leg}")


# ---- 3. factorised steps among refreshed ones: both LDS images in one step ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", ["rxc", "dense"])
@pytest.mark.parametrize("min_N", [2, 5])
@pytest.mark.parametrize("pd_stride", PD_LOW)
def test_pd_checks_below_the_horizon(pd_stride, min_N, leg):
    dense, rx_const = LEGS[leg]
    got = run(11, min_N, dense, "raw", rx_const, pd_stride=pd_stride)
    assert_form(got, "raw", rxc=rx_const)
    assert_oracle(got, reference(11, min_N, dense, pd_stride), f"pd_stride {pd_stride} every {min_N} {leg}")


# ---- 4. the shapes with one live register: Qs = (Qzz + Qzz')/2 ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pd_stride", [100, 3])
@pytest.mark.parametrize("leg", ["rxc", "dense"])
@pytest.mark.parametrize("task", SMALL)
def test_small_shapes_against_the_oracle(task, leg, pd_stride):
    dense, rx_const = LEGS[leg]
    got = run(11, 5, dense, "raw", rx_const, pd_stride=pd_stride, task=task)
    assert_form(got, "raw", rxc=rx_const)
    assert_oracle(got, reference(11, 5, dense, pd_stride, task=task), f"{task} {leg} pd_stride {pd_stride}")


# ---- 5. the gated and the listed twin -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(RETRY))
def test_gated_twin_under_a_failing_first_attempt(leg):
    p, refs = retry_problem(leg), retry_reference(leg)
    with fresh_engine(p) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=LEGS[leg][1])
        e.set_lambda_retry()
        st, dJ = e.backward(p["lam0"], pd_stride=RETRY_PD)
        lam_used, att = e.lambda_retry()
        K, k = e.gains()
        lb = e.last_launch("backward")
    assert ":w1:raw:uni" in lb and ((":rxc" in lb) == LEGS[leg][1]), lb
    print(f"gated {leg}: status {list(st)} attempts {list(att)} lambda_used {list(lam_used)}")
    assert list(att) == [len(r["visited"]) for r in refs] and max(att) > 1
    assert list(lam_used) == [r["lam"] for r in refs]
    for b, r in enumerate(refs):
        o = r["out"]
        assert st[b] == o["status"] == 0, (b, st[b], o["status"])
        fig = dict(K=relerr(K[b], o["K"]), k=relerr(k[b], o["k"]), delta_J=abs(dJ[b] - o["delta_J"]) / abs(o["delta_J"]))
        print(f"   b={b} lambda {r['lam']!r}: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
        assert all(v < RTOL for v in fig.values()), (b, fig)


@gpu
@pytest.mark.parametrize("leg", ["rxc", "dense"])
def test_listed_twin_on_a_scattered_subset(leg):
    dense, rx_const = LEGS[leg]
    p = problem(11, 5, dense, batch=LISTED_BATCH)
    refs = reference(11, 5, dense, batch=LISTED_BATCH)
    with fresh_engine(p) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=rx_const)
        st, dJ = e.backward_partial(LISTED, p["lam"])
        K, k = e.gains()
        lb = e.last_launch("backward")
    assert ":w1:" in lb and ":uni" in lb and lb.endswith(":subset") and ((":rxc" in lb) == rx_const), lb
    for i, b in enumerate(LISTED):
        o = refs[b]
        assert st[i] == o["status"] == 0, (b, st[i], o["status"])
        fig = dict(K=relerr(K[b], o["K"]), k=relerr(k[b], o["k"]), delta_J=abs(dJ[i] - o["delta_J"]) / abs(o["delta_J"]))
        print(f"listed {leg} b={b}: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
        assert all(v < RTOL for v in fig.values()), (b, fig)


# ---- 6. the uniform form against the general form, which keeps the transposition behind the product ----------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
def test_uniform_form_against_the_general_form(leg):
    dense, rx_const = LEGS[leg]
    uni = run(11, 5, dense, "raw", rx_const)
    gen = run(11, 5, dense, "raw", rx_const, general=True)
    assert_form(uni, "raw"); assert_form(gen, "raw", general=True)
    fig = figures(uni, gen)
    print(f"uniform vs general {leg}: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    assert np.array_equal(uni["status"], gen["status"])
    assert all(v < FTOL for v in fig.values()), fig


# ---- 7. the inputs (CPU) -----------------------------------------------------------------------------------------------------------------------
def test_inputs_succeed_on_the_oracle():
    """every input on which a GPU test above asserts success has status 0 on the oracle, and the retry problem has both outcomes"""
    for T in HORIZONS:
        for min_N in INTERVALS:
            for dense in (False, True):
                assert all(o["status"] == 0 for o in reference(T, min_N, dense)), (T, min_N, dense)
    for dense in (False, True):
        for lam in LAMBDAS:
            assert all(o["status"] == 0 for o in reference(11, 5, dense, lam=lam)), (lam, dense)
        for pd in PD_LOW:
            for min_N in (2, 5):
                assert all(o["status"] == 0 for o in reference(11, min_N, dense, pd)), (pd, min_N, dense)
        assert all(o["status"] == 0 for o in reference(11, 5, dense, batch=LISTED_BATCH)), dense
        for task in SMALL:
            for pd in (100, 3):
                assert all(o["status"] == 0 for o in reference(11, 5, dense, pd, task=task)), (task, pd, dense)
    assert len(LISTED) == 5 and LISTED_BATCH == 16 and np.any(np.diff(LISTED) > 1)
    for leg in RETRY:
        p, refs = retry_problem(leg), retry_reference(leg)
        first = [pipeline.run_trajectory(p, b, lam=float(p["lam0"][b]), pd_stride=RETRY_PD)["status"] for b in range(p["batch"])]
        assert any(s > 0 for s in first) and any(s == 0 for s in first), (leg, first)
        assert all(r["out"]["status"] == 0 for r in refs), (leg, [r["out"]["status"] for r in refs])
        assert [len(r["visited"]) > 1 for r in refs] == [s > 0 for s in first], leg
