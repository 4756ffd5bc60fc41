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
import numpy as np
import pytest

from _one_wave_backward import (LEGS, RETRY, assert_form, assert_forms_agree, assert_oracle, check_gated_twin, check_listed_twin,
                                check_retry_outcomes_on_the_oracle, check_uniform_against_general, problem, reference, run)

gpu = pytest.mark.gpu

PANDA = "panda_reaching"
HORIZONS = (2, 3, 11)
INTERVALS = (1, 2, 5)                                        # key-points every min_N steps
LAMBDAS = (1e-4, 10.0)
PD_LOW = (2, 3)
SMALL = ("acrobot", "hopper", "pentabot")                    # (4,1), (12,3), (10,3): NCU = 1, Qzz whole
LISTED_BATCH, LISTED = 16, [1, 6, 7, 12, 15]                 # the listed twin: a scattered subset


# ---- 1. Panda (14,7) at small horizons: every interval, payload and Jacobian leg --------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("min_N", INTERVALS)
@pytest.mark.parametrize("T", HORIZONS)
def test_panda_sweep_against_the_oracle(T, min_N, payload, leg):
    dense, rx_const = LEGS[leg]
    got = run(PANDA, T, min_N, dense, payload, rx_const)
    assert_form(got, payload, rxc=rx_const)
    assert_oracle(got, reference(PANDA, T, min_N, dense), f"T={T} every {min_N} {payload} {leg}")


@gpu
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("min_N", INTERVALS)
@pytest.mark.parametrize("T", HORIZONS)
def test_constant_jacobian_leg_against_the_per_step_leg(T, min_N, payload):
    rxc, per = run(PANDA, T, min_N, False, payload, True), run(PANDA, T, min_N, False, payload, False)
    assert_form(rxc, payload, rxc=True); assert_form(per, payload, rxc=False)
    assert_forms_agree(rxc, per, f"T={T} every {min_N} {payload} rxc vs per-step")


# ---- 2. lambda at both ends of the reference's range ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("lam", LAMBDAS)
def test_lambda_at_both_ends(lam, leg):
    dense, rx_const = LEGS[leg]
    got = run(PANDA, 11, 5, dense, "raw", rx_const, lam=lam)
    assert_form(got, "raw", rxc=rx_const)
    assert_oracle(got, reference(PANDA, 11, 5, dense, lam=lam), f"lambda {lam:g} {leg}")


# ---- 3. factorised steps among refreshed ones: both LDS images in one step ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", ["rxc", "dense"])
@pytest.mark.parametrize("min_N", [2, 5])
@pytest.mark.parametrize("pd_stride", PD_LOW)
def test_pd_checks_below_the_horizon(pd_stride, min_N, leg):
    dense, rx_const = LEGS[leg]
    got = run(PANDA, 11, min_N, dense, "raw", rx_const, pd_stride=pd_stride)
    assert_form(got, "raw", rxc=rx_const)
    assert_oracle(got, reference(PANDA, 11, min_N, dense, pd_stride), f"pd_stride {pd_stride} every {min_N} {leg}")


# ---- 4. the shapes with one live register: Qs = (Qzz + Qzz')/2 ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pd_stride", [100, 3])
@pytest.mark.parametrize("leg", ["rxc", "dense"])
@pytest.mark.parametrize("task", SMALL)
def test_small_shapes_against_the_oracle(task, leg, pd_stride):
    dense, rx_const = LEGS[leg]
    got = run(task, 11, 5, dense, "raw", rx_const, pd_stride=pd_stride)
    assert_form(got, "raw", rxc=rx_const)
    assert_oracle(got, reference(task, 11, 5, dense, pd_stride), f"{task} {leg} pd_stride {pd_stride}")


# ---- 5. the gated and the listed twin -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(RETRY))
def test_gated_twin_under_a_failing_first_attempt(leg):
    check_gated_twin(leg)


@gpu
@pytest.mark.parametrize("leg", ["rxc", "dense"])
def test_listed_twin_on_a_scattered_subset(leg):
    dense, rx_const = LEGS[leg]
    p = problem(PANDA, 11, 5, dense, batch=LISTED_BATCH)
    refs = reference(PANDA, 11, 5, dense, batch=LISTED_BATCH)
    check_listed_twin(p, refs, LISTED, rx_const, f"listed {leg}")


# ---- 6. the uniform form against the general form, which keeps the transposition behind the product ----------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
def test_uniform_form_against_the_general_form(leg):
    dense, rx_const = LEGS[leg]
    check_uniform_against_general(f"uniform vs general {leg}", PANDA, 11, 5, dense, rx_const)


# ---- 7. the inputs (CPU) -----------------------------------------------------------------------------------------------------------------------
def test_inputs_succeed_on_the_oracle():
    """every input on which a GPU test above asserts success has status 0 on the oracle, and the retry problem has both outcomes"""
    for T in HORIZONS:
        for min_N in INTERVALS:
            for dense in (False, True):
                assert all(o["status"] == 0 for o in reference(PANDA, T, min_N, dense)), (T, min_N, dense)
    for dense in (False, True):
        for lam in LAMBDAS:
            assert all(o["status"] == 0 for o in reference(PANDA, 11, 5, dense, lam=lam)), (lam, dense)
        for pd in PD_LOW:
            for min_N in (2, 5):
                assert all(o["status"] == 0 for o in reference(PANDA, 11, min_N, dense, pd)), (pd, min_N, dense)
        assert all(o["status"] == 0 for o in reference(PANDA, 11, 5, dense, batch=LISTED_BATCH)), dense
        for task in SMALL:
            for pd in (100, 3):
                assert all(o["status"] == 0 for o in reference(task, 11, 5, dense, pd)), (task, pd, dense)
    assert len(LISTED) == 5 and LISTED_BATCH == 16 and np.any(np.diff(LISTED) > 1)
    check_retry_outcomes_on_the_oracle()
