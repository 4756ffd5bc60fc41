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
import numpy as np
import pytest

from trajoptkp_amd import synth

import _lambda_retry as lr
from _one_wave_backward import (LEGS, RTOL, assert_bit_identical, assert_form, assert_forms_agree, assert_oracle, backward_figures,
                                check_uniform_against_general, fresh_engine, problem, reference, run, show)

gpu = pytest.mark.gpu

SIZES = {"T61": (61, 5), "T47": (47, 4), "T33": (33, 1)}          # T, min_N
PD_LOW = 7


def case(size, dense):
    """-> the arguments of problem(), reference() and run() for a size"""
    args = ("panda_reaching", *SIZES[size], dense)
    p = problem(*args)
    assert np.any(p["job_mode"][p["job_col"] >= p["n"]] != 0)          # one-sided CONTROL jobs are among them
    return args


@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_packed_sweep_against_the_oracle(size, payload, leg):
    dense, rx_const = LEGS[leg]
    got = run(*case(size, dense), payload, rx_const)
    assert_form(got, payload, rxc=rx_const)
    assert_oracle(got, reference(*case(size, dense)), f"{size} {payload} {leg}")


@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("size", sorted(SIZES))
def test_payloads_agree_bit_for_bit(size, leg):
    dense, rx_const = LEGS[leg]
    assert_bit_identical(run(*case(size, dense), "raw", rx_const), run(*case(size, dense), "kpc", rx_const))


@gpu
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_constant_jacobian_leg_against_the_per_step_leg(size, payload):
    rxc, per = run(*case(size, False), payload, True), run(*case(size, False), payload, False)
    assert_form(rxc, payload, rxc=True); assert_form(per, payload, rxc=False)
    assert_forms_agree(rxc, per, f"{size} {payload} rxc vs per-step")


@gpu
@pytest.mark.parametrize("payload,leg", [("raw", "rxc"), ("kpc", "dense"), ("raw", "dense")])
def test_pd_checks_below_the_horizon(payload, leg):
    """every 7th step is factorised from the tile whose columns 8..14 are not Quu's"""
    dense, rx_const = LEGS[leg]
    got = run(*case("T61", dense), payload, rx_const, pd_stride=PD_LOW)
    assert_form(got, payload, rxc=rx_const)
    assert_oracle(got, reference(*case("T61", dense), PD_LOW), f"pd_stride {PD_LOW} {payload} {leg}")


@gpu
@pytest.mark.parametrize("payload", ["raw", "kpc"])
def test_negative_running_weights_fail_where_the_oracle_fails(payload):
    p = lr.problem("panda")
    refs = [lr.sweep("panda", None, b, float(p["lam0"][b])) for b in range(p["batch"])]
    with fresh_engine(p) as e:
        synth.upload(e, p, kp_ordered=(payload == "raw"))
        st, dJ = e.backward(p["lam0"], pd_stride=lr.PD_STRIDE)
        K, k = e.gains()
        lb = e.last_launch("backward")
    assert_form(lb, payload)
    want = [o["status"] for o in refs]
    print(f"negative weights {payload}: status {list(st)} oracle {want}")
    assert list(st) == want
    assert any(s > 0 for s in want) and any(s == 0 for s in want)
    for b, o in enumerate(refs):
        if o["status"] == 0:
            fig = backward_figures(K[b], k[b], dJ[b], o)
            print(f"   b={b}: {show(fig)}")
            assert all(v < RTOL for v in fig.values()), (b, fig)


@gpu
def test_uniform_form_against_the_general_form():
    check_uniform_against_general("uniform vs general", *case("T61", False), True)


def test_inputs_succeed_on_the_oracle():
    """(CPU) every input on which a GPU test above asserts success has status 0 on the oracle, and the negative-weight problem has
    both outcomes"""
    for size in SIZES:
        for dense in (False, True):
            assert all(o["status"] == 0 for o in reference(*case(size, dense))), (size, dense)
    for dense in (False, True):
        assert all(o["status"] == 0 for o in reference(*case("T61", dense), PD_LOW)), dense
    p = lr.problem("panda")
    st = [lr.sweep("panda", None, b, float(p["lam0"][b]))["status"] for b in range(p["batch"])]
    assert any(s > 0 for s in st) and any(s == 0 for s in st), st
