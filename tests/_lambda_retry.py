"""Shared by tests/test_lambda_retry_model.py (CPU) and tests/test_gpu_lambda_retry.py: the problems of the lambda retry tests, the
kernel-family cases that run them, and the reference loop -- the failure side of the reference's lambda schedule (iLQR.cpp:435-442,
UpdateLambda :636-657) composed from the oracle's backward pass, per trajectory:

    sweep at lambda; status == 0: settled.  Otherwise lambda' = lambda * factor; lambda' > max_lambda: give up; otherwise, while
    fewer than max_attempts sweeps have run, sweep again at lambda'.

With factor 10 the step is orc.update_lambda (the oracle's UpdateLambda); with any other factor it is lam * factor directly.

Inputs that fail PD checks: dense residual Jacobians and NEGATIVE running weights, w_run = -(|w_run| + 1) * s, so that l_uu is
negative definite and Q_uu + lambda I fails its Cholesky test until lambda outweighs it; pd_stride = 10, so a sweep can fail
mid-horizon.  Every problem runs with the per-trajectory start lambdas LAM0[:batch]: within one batch some trajectories settle at
once, some after several attempts, and (acrobot, arm8) some give up.  The scales s were found with `python tests/_lambda_retry.py`,
which prints the attempts of a range of scales per problem; test_lambda_retry_model.py asserts what the GPU tests rely on.

Conditioning.  A sweep that settles with Q_uu + lambda I barely positive definite has gains that amplify rounding: the GPU sweeps
and the oracle associate their products differently, so they agree to about S * 1e-15, S being the relative change of K per relative
change of lambda (sensitivity() below, measured on the oracle alone).  The 1e-9 bar of the suite therefore needs S well below 1e6;
test_lambda_retry_model.py holds every settled sweep the GPU tests compare to S <= MAX_SENSITIVITY = 1e5 (a scale at which
`pushing` settled at S = 4e7 under the factor-4 schedule was replaced for that reason, before any GPU figure was looked at again).
Everything here is computed once per process and shared; nothing is ever modified."""
import functools

import numpy as np

from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import synth

PD_STRIDE = 10
FACTOR, MAX_LAMBDA, MAX_ATTEMPTS = 10.0, 10.0, 6              # Engine.set_lambda_retry's defaults
LAM0 = (0.1, 1.0, 10.0, 1e-4, 0.1, 10.0)
OTHER_SCHEDULE = dict(factor=4.0, max_lambda=50.0, max_attempts=8)      # the second schedule of the GPU tests
MAX_SENSITIVITY = 1e5

# name: (task, T, batch, s, ragged)
PROBLEMS = {
    "panda": ("panda_reaching", 64, 4, 20.0, False),
    "panda_ragged": ("panda_reaching", 64, 4, 20.0, True),
    "acrobot": ("acrobot", 48, 5, 3.0, False),
    "pushing": ("panda_pushing", 48, 4, 12.0, False),
    "clutter": ("light_clutter_push", 32, 4, 20.0, False),
    "arm8": ("arm8", 48, 6, 55.0, False),
    "quadruped": ("quadruped", 48, 4, 20.0, False),
}
GIVE_UP = ("acrobot", "arm8")          # a one-tile and a tiled problem in which a trajectory gives up

# Kernel families: name -> (problem, Engine keywords, environment read when the context is created, key-point ordered payload,
# what kpilqr_last_launch(backward) has to contain)
CASES = {
    "fused_w1_kpc": ("panda", dict(fused=True), {"KPILQR_FUSED_WAVES": "1"}, False, ":w1:kpc:uni"),
    "fused_w1_raw": ("panda", dict(fused=True), {"KPILQR_FUSED_WAVES": "1"}, True, ":w1:raw:uni"),
    "fused_pair_raw": ("panda", dict(fused=True), {"KPILQR_FUSED_WAVES": "5"}, True, ":pairh:raw:uni"),
    "fused_pair_shift0": ("panda", dict(fused=True), {"KPILQR_FUSED_WAVES": "5", "KPILQR_ROLE_SHIFT": "0"}, False, ":pairh:kpc:uni"),
    "fused_w1_ragged": ("panda_ragged", dict(fused=True), {"KPILQR_FUSED_WAVES": "1"}, True, ":w1:"),
    "fused_pair_ragged": ("panda_ragged", dict(fused=True), {"KPILQR_FUSED_WAVES": "5"}, False, ":pairh:"),
    "fused_union": ("panda_ragged", dict(fused=True, union_keypoints=True), {"KPILQR_FUSED_WAVES": "1"}, True, ":union"),
    "fused_acrobot": ("acrobot", dict(fused=True), {"KPILQR_FUSED_WAVES": "1"}, True, ":w1:raw:uni"),
    "t1": ("panda", dict(), {}, False, "mfma_f64_t1"),
    "t1_acrobot": ("acrobot", dict(), {}, True, "mfma_f64_t1"),
    "tiled_uw": ("pushing", dict(), {}, False, "mfma_f64_tiled"),
    "tiled_col": ("pushing", dict(), {"KPILQR_TILED_UW": "0"}, True, "mfma_f64_tiled"),
    "tiled_a6": ("pushing", dict(fused=True), {"KPILQR_TILED_A6": "1"}, True, "mfma_f64_tiled_a6"),
    "tiled_3": ("clutter", dict(), {}, False, "mfma_f64_tiled"),
    "tiled_pad8": ("arm8", dict(), {}, False, "mfma_f64_tiled"),
    "wide": ("quadruped", dict(), {}, False, "mfma_f64_wide"),
    "generic": ("acrobot", dict(generic=True), {}, False, "generic_lds"),
    "generic_panda": ("panda", dict(generic=True), {}, True, "generic_lds"),
}


def _ragged_rows(seed, dof, T, batch):
    """per-DoF key-point lists (recursive bisection, synth.bisect_keypoints), different for every DoF and trajectory"""
    rng = np.random.default_rng(seed)
    return [synth.bisect_keypoints(rng, dof, T, 3, rng.uniform(0.3, 0.95, dof)) for _ in range(batch)]


@functools.lru_cache(maxsize=None)
def problem(name, s=None):
    task, T, batch, s0, ragged = PROBLEMS[name]
    s = s0 if s is None else s
    if ragged:
        p = synth.make_ragged_problem(task, T, _ragged_rows(41, synth.TASKS[task]["dof"], T, batch), config_id=21, dense_residuals=True)
    else:
        p = synth.make_problem(task=task, T=T, batch=batch, min_N=5, dense_residuals=True)
    p["w_run"] = -(np.abs(p["w_run"]) + 1.0) * s
    p["lam0"] = np.array(LAM0[:batch])
    return p


@functools.lru_cache(maxsize=None)
def sweep(name, s, b, lam):
    """the oracle's whole iteration of trajectory b at lambda `lam` (backward pass with the PD checks, forward pass when it is valid)"""
    return pipeline.run_trajectory(problem(name, s), b, lam=lam, pd_stride=PD_STRIDE)


def next_lambda(lam, factor, max_lambda):
    """-> (lambda', give up): the failing branch of UpdateLambda"""
    if factor == 10.0:
        nxt, ex = orc.update_lambda(lam, False, 10.0, 1e-4, max_lambda)
        return (lam * factor if ex else nxt), ex          # (the oracle clamps at the exit; the multiply is the same)
    nxt = lam * factor
    return nxt, nxt > max_lambda


@functools.lru_cache(maxsize=None)
def reference(name, lam0=None, factor=FACTOR, max_lambda=MAX_LAMBDA, max_attempts=MAX_ATTEMPTS, s=None):
    """The reference loop over every trajectory of a problem from the start lambdas lam0 (a tuple; default: the problem's).
    -> dict: status, lambda_used, attempts [batch]; visited: the lambdas swept, per trajectory; settled: status == 0;
    gave_up: failed and lambda_used * factor > max_lambda; out: the oracle's results of every trajectory's LAST sweep."""
    p = problem(name, s)
    B = p["batch"]
    lam0 = tuple(p["lam0"]) if lam0 is None else tuple(lam0)
    status = np.zeros(B, np.int32); used = np.zeros(B); attempts = np.zeros(B, np.int32); gave_up = np.zeros(B, bool)
    visited, outs = [], []
    for b in range(B):
        lam, seen = float(lam0[b]), []
        while True:
            o = sweep(name, s, b, lam)
            seen.append(lam)
            if o["status"] == 0:
                break
            nxt, ex = next_lambda(lam, factor, max_lambda)
            if ex:
                gave_up[b] = True
                break
            if len(seen) >= max_attempts:
                break
            lam = nxt
        status[b], used[b], attempts[b] = o["status"], lam, len(seen)
        visited.append(tuple(seen)); outs.append(o)
    return dict(status=status, lambda_used=used, attempts=attempts, visited=tuple(visited), settled=status == 0, gave_up=gave_up, out=tuple(outs))


@functools.lru_cache(maxsize=None)
def sensitivity(name, b, lam, s=None):
    """relative change of K per relative change of lambda at a settled sweep, on the oracle (inf: the perturbed sweep fails)"""
    o = sweep(name, s, b, lam)
    q = pipeline.run_trajectory(problem(name, s), b, lam=lam * (1.0 + 2.0 ** -40), pd_stride=PD_STRIDE)
    if o["status"] != 0 or q["status"] != 0:
        return float("inf")
    return float(np.max(np.abs(q["K"] - o["K"])) / np.max(np.abs(o["K"])) / 2.0 ** -40)


if __name__ == "__main__":          # how the scales of PROBLEMS were found
    for name in PROBLEMS:
        for s in (0.1, 0.5, 3.0, 20.0, 100.0):
            r = reference(name, s=s)
            print(f"{name:14s} s={s:6.1f} attempts {list(r['attempts'])} status {list(r['status'])} gave up {list(r['gave_up'].astype(int))}", flush=True)
