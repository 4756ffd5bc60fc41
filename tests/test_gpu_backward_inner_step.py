"""The inner step of the uniform one-wave backward sweep (fused_mfma.hip, `UNI && !PC`): what it carries from step to step and where
the cost block joins V'.

  * HEADS, every uniform one-wave shape: the running inverse, the one before it and the gains waiting to be stored are their NCU live
    registers (NCU = 2 at (14,7), 1 for hopper, pentabot, acrobot); the first guess of every refresh is written into the head of a tile
    whose zero tail was set up once (kp_inverse_refresh_heads); a factorised step re-seeds heads only, and the step behind it
    extrapolates from Xprev = Xinv.
  * MRG, (14,7): Lzz joins the halved merged tile of V' = Qm + K'G by four FMAs behind the D products, whose accumulators start from
    lambda I and zero (from l_uu + lambda I and l_uz with control residuals); with a constant r_x the deposit of l_x is one product on the
    halved constant tile at the top of the step; V = acc + acc' without a 0.5.  The terminal step (V = Lzz) keeps its full product and halves it for the merge.

The shapes are the smallest at which those statements can go wrong: T = 2 is the terminal step plus one, key-points every 1, 2 and 5
steps make every step a peeled one, peeled and inner steps alternate, and the headline's segment of four inner steps; pd_stride 2 and 3
put a factorisation (a re-seed) in front of a peeled and of an inner step.  Legs: the constant residual Jacobian (`:rxc`), the same
matrix given per step (within 1e-12 of it), dense per-step Jacobians with r_u != 0; payloads: key-point ordered (`raw`: the sweep
differences) and job lists (`kpc`), equal bit for bit.  The gated twin runs under a lambda retry schedule whose first lambda fails on
the oracle for some trajectories and whose second does not; the listed twin sweeps a scattered subset.
(The launch string has no token for the gated twin: that it ran is inferred from attempts > 1.  A refresh that GIVES UP is not provoked
by these inputs -- their residuals stay far below 0.11 -- and nothing here asserts one: the step after a give-up re-seeds through the
same statements as the step after a checked step, which pd_stride 2 and 3 reach; the give-up sequences themselves are
tests/test_gpu_refresh.py's.)

Everything is held to oracle.pipeline.run_trajectory at 1e-9 (K, k, delta_J, predicted costs; status exactly), forms of one sweep to
each other at 1e-12.  The oracle's runs are made once per problem and shared; the CPU test at the bottom asserts that every input on
which success is asserted succeeds on the oracle, and that the retry problem has both outcomes."""
import pytest

from _one_wave_backward import (LEGS, RETRY, assert_bit_identical, assert_form, assert_forms_agree, assert_oracle, check_gated_twin,
                                check_listed_twin, check_retry_outcomes_on_the_oracle, check_uniform_against_general, problem, reference, run)

gpu = pytest.mark.gpu

HORIZONS = (2, 3, 4, 6, 11)
INTERVALS = (1, 2, 5)                                        # key-points every min_N steps
SMALL = {"hopper": "hopper", "pentabot": "pentabot", "acrobot": "acrobot"}                  # (12,3), (10,3), (4,1): NCU = 1
PD_LOW = (2, 3)
LISTED = [0, 2, 4]                                           # the listed twin: a scattered subset of five trajectories


# ---- 1. Panda (14,7): every horizon, interval, leg and payload --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("min_N", INTERVALS)
@pytest.mark.parametrize("T", HORIZONS)
def test_panda_sweep_against_the_oracle(T, min_N, payload, leg):
    dense, rx_const = LEGS[leg]
    got = run("panda_reaching", T, min_N, dense, payload, rx_const)
    assert_form(got, payload, rxc=rx_const)
    assert_oracle(got, reference("panda_reaching", T, min_N, dense), f"T={T} every {min_N} {payload} {leg}")


@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("min_N", INTERVALS)
@pytest.mark.parametrize("T", HORIZONS)
def test_payloads_agree_bit_for_bit(T, min_N, leg):
    dense, rx_const = LEGS[leg]
    assert_bit_identical(run("panda_reaching", T, min_N, dense, "raw", rx_const), run("panda_reaching", T, min_N, dense, "kpc", rx_const))


@gpu
@pytest.mark.parametrize("payload", ["raw", "kpc"])
@pytest.mark.parametrize("min_N", INTERVALS)
@pytest.mark.parametrize("T", HORIZONS)
def test_constant_jacobian_leg_against_the_per_step_leg(T, min_N, payload):
    rxc, per = run("panda_reaching", T, min_N, False, payload, True), run("panda_reaching", T, min_N, False, payload, False)
    assert_form(rxc, payload, rxc=True); assert_form(per, payload, rxc=False)
    assert_forms_agree(rxc, per, f"T={T} every {min_N} {payload} rxc vs per-step")


# ---- 2. factorised steps among refreshed ones: the re-seed hands back heads ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", ["rxc", "dense"])
@pytest.mark.parametrize("min_N", [2, 5])
@pytest.mark.parametrize("pd_stride", PD_LOW)
def test_pd_checks_below_the_horizon(pd_stride, min_N, leg):
    dense, rx_const = LEGS[leg]
    got = run("panda_reaching", 11, min_N, dense, "raw", rx_const, pd_stride=pd_stride)
    assert_form(got, "raw", rxc=rx_const)
    assert_oracle(got, reference("panda_reaching", 11, min_N, dense, pd_stride), f"pd_stride {pd_stride} every {min_N} {leg}")


# ---- 3. the shapes with one live register ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", ["rxc", "dense"])
@pytest.mark.parametrize("min_N", [1, 5])
@pytest.mark.parametrize("T", [3, 11])
@pytest.mark.parametrize("task", sorted(SMALL))
def test_small_shapes_against_the_oracle(task, T, min_N, leg):
    dense, rx_const = LEGS[leg]
    got = run(SMALL[task], T, min_N, dense, "raw", rx_const)
    assert_form(got, "raw", rxc=rx_const)
    assert_oracle(got, reference(SMALL[task], T, min_N, dense), f"{task} T={T} every {min_N} {leg}")


@gpu
@pytest.mark.parametrize("task", sorted(SMALL))
def test_small_shapes_with_pd_checks_below_the_horizon(task):
    got = run(SMALL[task], 11, 5, False, "raw", True, pd_stride=3)
    assert_form(got, "raw", rxc=True)
    assert_oracle(got, reference(SMALL[task], 11, 5, False, 3), f"{task} pd_stride 3")


# ---- 4. the gated and the listed twin -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(RETRY))
def test_gated_twin_under_a_lambda_retry_schedule(leg):
    check_gated_twin(leg)


@gpu
@pytest.mark.parametrize("leg", ["rxc", "dense"])
def test_listed_twin_on_a_scattered_subset(leg):
    dense, rx_const = LEGS[leg]
    p = problem("panda_reaching", 11, 5, dense, batch=5)
    refs = reference("panda_reaching", 11, 5, dense, batch=5)
    check_listed_twin(p, refs, LISTED, rx_const, f"listed {leg}")


# ---- 5. the uniform form against the general form, which keeps its statements --------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leg", sorted(LEGS))
def test_uniform_form_against_the_general_form(leg):
    dense, rx_const = LEGS[leg]
    check_uniform_against_general(f"uniform vs general {leg}", "panda_reaching", 11, 5, dense, rx_const)


# ---- 6. the inputs (CPU) -----------------------------------------------------------------------------------------------------------------------
def test_inputs_succeed_on_the_oracle():
    """every input on which a GPU test above asserts success has status 0 on the oracle, and the retry problem has both outcomes"""
    for T in HORIZONS:
        for min_N in INTERVALS:
            for dense in (False, True):
                assert all(o["status"] == 0 for o in reference("panda_reaching", T, min_N, dense)), (T, min_N, dense)
    for pd in PD_LOW:
        for min_N in (2, 5):
            for dense in (False, True):
                assert all(o["status"] == 0 for o in reference("panda_reaching", 11, min_N, dense, pd)), (pd, min_N, dense)
    for task in SMALL.values():
        for T in (3, 11):
            for min_N in (1, 5):
                for dense in (False, True):
                    assert all(o["status"] == 0 for o in reference(task, T, min_N, dense)), (task, T, min_N, dense)
        assert all(o["status"] == 0 for o in reference(task, 11, 5, False, 3)), task
    for dense in (False, True):
        assert all(o["status"] == 0 for o in reference("panda_reaching", 11, 5, dense, batch=5)), dense
    check_retry_outcomes_on_the_oracle()
