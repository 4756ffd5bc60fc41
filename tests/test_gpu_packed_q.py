"""The packed Q products of the uniform one-wave backward sweep at (14,7) (fused_mfma.hip, PACKQ): Quu, Quz and the needed entries of
Qzz come out of two products on packed operand tiles, whose lanes 8..14 walk a SECOND key-point column (B column c - 8 of DoF c - 8)
beside their own A column.  What can go wrong is in the tracker of those lanes and in the blocks nobody computes any more:

  * one-sided control jobs (one_sided_frac): the duplicated B lanes take the exceptional differencing branch with the control bit of
    another DoF's mode word;
  * a short last segment (T=47, min_N=4) and a crossing on every step (T=33, min_N=1);
  * the key-point ordered payload (`raw`: the sweep differences, and must not store the duplicated columns) and job lists (`kpc`):
    K and the predicted costs of the two are equal bit for bit;
  * the constant residual Jacobian (`:rxc`: the 2 e_n v' deposit lands on the merged tile), the same matrix given per step (within
    1e-12 of it) and dense per-step Jacobians with r_u != 0 (l_uu and l_uz ride in the accumulators' initial values);
  * a PD-check stride below T (7, the stride of tests/test_gpu_refresh.py): the LDL' path reads Quu from a tile whose columns 8..14
    are not masked;
  * negative running weights (tests/_lambda_retry.py's panda problem): failing status and step are the oracle's;
  * the uniform form against the general per-DoF-list form (KPILQR_FUSED_UNI=0), which keeps its three products, at 1e-12.

Everything is held to oracle.pipeline.run_trajectory at 1e-9 (K, k, delta_J, predicted costs; status exactly).  hopper (12,3) and
pentabot (10,3) keep their products and are not cases here.  The oracle's runs are made once per problem and shared; the CPU test
at the bottom asserts that every input on which success is asserted succeeds on the oracle."""
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
SIZES = {"T61": (61, 5), "T47": (47, 4), "T33": (33, 1)}          # T, min_N
PD_LOW = 7


@functools.lru_cache(maxsize=None)
def problem(size, dense):
    T, min_N = SIZES[size]
    p = synth.make_problem(task="panda_reaching", T=T, batch=BATCH, min_N=min_N, one_sided_frac=0.25, dense_residuals=dense)
    assert np.any(p["job_mode"][p["job_col"] >= p["n"]] != 0)          # one-sided CONTROL jobs are among them
    return p


@functools.lru_cache(maxsize=None)
def reference(size, dense, pd_stride=100):
    p = problem(size, dense)
    return [pipeline.run_trajectory(p, b, pd_stride=pd_stride) for b in range(p["batch"])]


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


@pytest.fixture(autouse=True)
def one_wave(monkeypatch):
    monkeypatch.delenv("KPILQR_FUSED_UNI", raising=False)
    monkeypatch.setenv("KPILQR_FUSED_WAVES", "1")
    monkeypatch.setenv("KPILQR_FUSED_FWD_WAVES", "1")


@functools.lru_cache(maxsize=None)
def run(size, dense, payload, rx_const, pd_stride=100, general=False):
    """One kpilqr_iterate of the problem on a fresh context (the environment is read when it is created)."""
    p = problem(size, dense)
    if general:
        os.environ["KPILQR_FUSED_UNI"] = "0"
    try:
        e = Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=True)
    finally:
        os.environ.pop("KPILQR_FUSED_UNI", None)
    with e:
        synth.upload(e, p, kp_ordered=(payload == "raw"), rx_const=rx_const)
        e.iterate(p["lam"], pd_stride, ALPHAS)
        res = e.results()
        K, k = e.gains()
        return dict(K=K, k=k, launch=e.last_launch("backward"), **res)


def assert_form(got, payload, rxc=None, general=False):
    lb = got["launch"]
    assert ":w1:" in lb and f":{payload}:" in lb, lb
    if general:
        assert ":uni" not in lb, lb
    else:
        assert ":uni" in lb, lb
    if rxc is not None:
        assert (":rxc" in lb) == rxc, lb


def figures(got, want, b=None):
    sl = slice(None) if b is None else b
    fig = dict(K=relerr(got["K"][sl], want["K"]), k=relerr(got["k"][sl], want["k"]),
               delta_J=abs(float(got["delta_J"][sl]) - float(want["delta_J"])) / abs(float(want["delta_J"])) if b is not None
               else relerr(got["delta_J"], want["delta_J"]),
               cost_pred=relerr(got["cost_pred"][sl], want["cost_pred"]))
    return fig


def assert_oracle(got, refs, label):
    for b, o in enumerate(refs):
        fig = figures(got, o, b)
        print(f"{label} b={b}: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
        assert got["status"][b] == o["status"] == 0, (label, b, got["status"][b], o["status"])
        assert all(v < RTOL for v in fig.values()), (label, b, fig)


LEGS = {"rxc": (False, True), "per_step": (False, False), "dense": (True, False)}          # dense residuals, constant-Jacobian upload


@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_packed_sweep_against_the_oracle(size, payload, leg):
    dense, rx_const = LEGS[leg]
    got = run(size, dense, payload, rx_const)
    assert_form(got, payload, rxc=rx_const)
    assert_oracle(got, reference(size, dense), f"{size} {payload} {leg}")


@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("size", sorted(SIZES))
def test_payloads_agree_bit_for_bit(size, leg):
    dense, rx_const = LEGS[leg]
    raw, kpc = run(size, dense, "raw", rx_const), run(size, dense, "kpc", rx_const)
    assert np.array_equal(raw["K"], kpc["K"]) and np.array_equal(raw["cost_pred"], kpc["cost_pred"])


@gpu
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_constant_jacobian_leg_against_the_per_step_leg(size, payload):
    rxc, per = run(size, False, payload, True), run(size, False, payload, False)
    assert_form(rxc, payload, rxc=True); assert_form(per, payload, rxc=False)
    fig = figures(rxc, per)
    print(f"{size} {payload} rxc vs per-step: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    assert np.array_equal(rxc["status"], per["status"])
    assert all(v < FTOL for v in fig.values()), fig


@gpu
@pytest.mark.parametrize("payload,leg", [("raw", "rxc"), ("kpc", "dense"), ("raw", "dense")])
def test_pd_checks_below_the_horizon(payload, leg):
    """every 7th step is factorised from the tile whose columns 8..14 are not Quu's"""
    dense, rx_const = LEGS[leg]
    got = run("T61", dense, payload, rx_const, pd_stride=PD_LOW)
    assert_form(got, payload, rxc=rx_const)
    assert_oracle(got, reference("T61", dense, PD_LOW), f"pd_stride {PD_LOW} {payload} {leg}")


@gpu
@pytest.mark.parametrize("payload", ["raw", "kpc"])
def test_negative_running_weights_fail_where_the_oracle_fails(payload):
    p = lr.problem("panda")
    refs = [lr.sweep("panda", None, b, float(p["lam0"][b])) for b in range(p["batch"])]
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=True) as e:
        synth.upload(e, p, kp_ordered=(payload == "raw"))
        st, dJ = e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        K, k = e.gains()
        lb = e.last_launch("backward")
    assert ":w1:" in lb and ":uni" in lb and f":{payload}:" in lb, lb
    want = [o["status"] for o in refs]
    print(f"negative weights {payload}: status {list(st)} oracle {want}")
    assert list(st) == want
    assert any(s > 0 for s in want) and any(s == 0 for s in want)
    for b, o in enumerate(refs):
        if o["status"] == 0:
            fig = dict(K=relerr(K[b], o["K"]), k=relerr(k[b], o["k"]), delta_J=abs(dJ[b] - o["delta_J"]) / abs(o["delta_J"]))
            print(f"   b={b}: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
            assert all(v < RTOL for v in fig.values()), (b, fig)


@gpu
def test_uniform_form_against_the_general_form():
    uni = run("T61", False, "raw", True)
    gen = run("T61", False, "raw", True, general=True)
    assert_form(uni, "raw"); assert_form(gen, "raw", general=True)
    fig = figures(uni, gen)
    print("uniform vs general: " + " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    assert np.array_equal(uni["status"], gen["status"])
    assert all(v < FTOL for v in fig.values()), fig


def test_inputs_succeed_on_the_oracle():
    """(CPU) every input on which a GPU test above asserts success has status 0 on the oracle, and the negative-weight problem has
    both outcomes"""
    for size in SIZES:
        for dense in (False, True):
            assert all(o["status"] == 0 for o in reference(size, dense)), (size, dense)
    for dense in (False, True):
        assert all(o["status"] == 0 for o in reference("T61", dense, PD_LOW)), dense
    p = lr.problem("panda")
    st = [lr.sweep("panda", None, b, float(p["lam0"][b]))["status"] for b in range(p["batch"])]
    assert any(s > 0 for s in st) and any(s == 0 for s in st), st
