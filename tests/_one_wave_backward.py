"""Shared by the test files of the uniform one-wave backward sweep (tests/test_gpu_packed_q.py, test_gpu_backward_factor_path.py,
test_gpu_backward_inner_step.py, test_gpu_backward_early_symmetrise.py): the problems, the oracle's runs, one kpilqr_iterate on a
fresh context, the checks of a launch string and of results against oracle.pipeline.run_trajectory, and the three test bodies the
files have in common (gated twin, listed twin, uniform against general form).  tests/test_one_wave_harness.py holds the checks
themselves to the oracle alone (no GPU).

Everything cached here is computed once per session and shared by every file: a case two files have in common is swept once on
the GPU and once on the oracle.  Nothing cached is ever modified.  A context reads the environment when it is created and never
again (kpilqr_create); sweep_env() is the only place that sets it, so the arguments of run() determine the context it ran on."""
import contextlib
import functools
import inspect
import os

import numpy as np

from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import Engine, synth

import _lambda_retry as lr

RTOL = 1e-9          # to the oracle
FTOL = 1e-12         # between forms of the same sweep
ALPHAS = orc.alphas(6)
LEGS = {"rxc": (False, True), "per_step": (False, False), "dense": (True, False)}          # dense residuals, constant-Jacobian upload
WAVE_KEYS = ("KPILQR_FUSED_WAVES", "KPILQR_FUSED_FWD_WAVES", "KPILQR_FUSED_UNI", "KPILQR_FUSED_RAW")

# the gated twin: Panda T = 11 under negative running weights, w_run = -(|w_run| + 1) * scale as tests/_lambda_retry.py makes
# sweeps fail (its own Panda problem has T = 64), a PD check every RETRY_PD steps.  On the oracle the constant-Jacobian leg (scale 20)
# fails at lambda 1e-4 and settles from 0.1 on, the dense leg (scale 3) fails at 0.1 and settles from 1 on, each a decade or more away
# from the edge (K moves by ~1 relative per relative change of lambda there: no conditioning to speak of).  Looked for on the oracle
# alone; the CPU tests of the files that run it assert what is relied on.
RETRY_PD, RETRY_BATCH = 3, 4
RETRY = {"rxc": (20.0, (1e-4, 0.1, 1e-4, 1.0)), "dense": (3.0, (0.1, 1.0, 10.0, 0.1))}          # leg: scale, start lambdas


def _cached(fn):
    """functools.lru_cache on the BOUND arguments: f(a, pd_stride=3), f(a, 3) and, where 3 is the default, f(a) are one entry"""
    sig = inspect.signature(fn)
    inner = functools.lru_cache(maxsize=None)(fn)

    @functools.wraps(fn)
    def call(*args, **kw):
        bound = sig.bind(*args, **kw)
        bound.apply_defaults()
        return inner(*bound.args)
    call.cache_info = inner.cache_info
    return call


# ---- problems and the oracle's runs -----------------------------------------------------------------------------------------------------
@_cached
def problem(task, T, min_N, dense, batch=3, lam=0.1, one_sided_frac=0.25):
    return synth.make_problem(task=task, T=T, batch=batch, min_N=min_N, one_sided_frac=one_sided_frac, dense_residuals=dense, lam=lam)


@_cached
def reference(task, T, min_N, dense, pd_stride=100, batch=3, lam=0.1, one_sided_frac=0.25):
    p = problem(task, T, min_N, dense, batch, lam, one_sided_frac)
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


# ---- contexts -------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def sweep_env(one_wave=True, general=False):
    """The environment a context is created under: none of WAVE_KEYS but what the case asks for -- the one-wave sweeps forced
    (KPILQR_FUSED_WAVES = KPILQR_FUSED_FWD_WAVES = 1), the general per-DoF-list form (KPILQR_FUSED_UNI = 0).  Restored on exit."""
    saved = {key: os.environ.pop(key, None) for key in WAVE_KEYS}
    if one_wave:
        os.environ["KPILQR_FUSED_WAVES"] = os.environ["KPILQR_FUSED_FWD_WAVES"] = "1"
    if general:
        os.environ["KPILQR_FUSED_UNI"] = "0"
    try:
        yield
    finally:
        for key, value in saved.items():
            os.environ.pop(key, None)
            if value is not None:
                os.environ[key] = value


def fresh_engine(p, one_wave=True, general=False):
    with sweep_env(one_wave, general):
        return Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=True)


@_cached
def run(task, T, min_N, dense, payload, rx_const, pd_stride=100, general=False, lam=0.1, batch=3, one_wave=True, one_sided_frac=0.25):
    """One kpilqr_iterate of problem(...) on a fresh context -> K, k, the results and the backward launch string."""
    p = problem(task, T, min_N, dense, batch, lam, one_sided_frac)
    with fresh_engine(p, one_wave, general) as e:
        synth.upload(e, p, kp_ordered=(payload == "raw"), rx_const=rx_const)
        e.iterate(p["lam"], pd_stride, ALPHAS)
        res = e.results()
        K, k = e.gains()
        return dict(K=K, k=k, launch=e.last_launch("backward"), **res)


# ---- checks -----------------------------------------------------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def show(fig):
    return " ".join(f"{n} {v:.2e}" for n, v in fig.items())


def assert_form(got, payload, rxc=None, general=False):
    """the backward launch string (or the results of run()): one wave, the payload, uniform or general form, constant Jacobian"""
    lb = got if isinstance(got, str) else got["launch"]
    assert ":w1:" in lb and f":{payload}:" in lb, lb
    assert (":uni" in lb) == (not general), lb
    if rxc is not None:
        assert (":rxc" in lb) == rxc, lb


def figures(got, want, b=None):
    """relative errors of K, k, delta_J and the predicted costs: trajectory b of `got` against one oracle run, or (b None) two
    whole results against each other"""
    sl = slice(None) if b is None else b
    return dict(K=relerr(got["K"][sl], want["K"]), k=relerr(got["k"][sl], want["k"]),
                delta_J=abs(float(got["delta_J"][sl]) - float(want["delta_J"])) / abs(float(want["delta_J"])) if b is not None
                else relerr(got["delta_J"], want["delta_J"]),
                cost_pred=relerr(got["cost_pred"][sl], want["cost_pred"]))


def assert_oracle(got, refs, label, rows=None, quiet=False):
    """Every oracle run of refs succeeds and so does its trajectory of `got` (refs[i] is trajectory rows[i]; all of them in order
    without rows), every figure < RTOL.  -> the worst figures."""
    worst = dict(K=0.0, k=0.0, delta_J=0.0, cost_pred=0.0)
    for i, o in enumerate(refs):
        b = i if rows is None else rows[i]
        fig = figures(got, o, b)
        worst = {n: max(worst[n], v) for n, v in fig.items()}
        if not quiet:
            print(f"{label} b={b}: {show(fig)}")
        assert got["status"][b] == o["status"] == 0, (label, b, got["status"][b], o["status"])
        assert all(v < RTOL for v in fig.values()), (label, b, fig)
    return worst


def assert_forms_agree(a, b, label):
    """two forms of the same sweep: the status equal, every figure < FTOL"""
    fig = figures(a, b)
    print(f"{label}: {show(fig)}")
    assert np.array_equal(a["status"], b["status"])
    assert all(v < FTOL for v in fig.values()), fig


def assert_bit_identical(a, b):
    """the two payloads of one sweep: gains, delta_J, predicted costs and status equal bit for bit"""
    for name in ("K", "k", "delta_J", "cost_pred", "status"):
        assert np.array_equal(a[name], b[name]), name


def backward_figures(K, k, dJ, o):
    """a backward sweep alone (no predicted costs): one trajectory's K, k and delta_J against its oracle run"""
    return dict(K=relerr(K, o["K"]), k=relerr(k, o["k"]), delta_J=abs(dJ - o["delta_J"]) / abs(o["delta_J"]))


def assert_backward_oracle(st, dJ, K, k, refs, rows, label):
    """st, dJ [len(rows)] of a backward call and the context's K, k [batch]: trajectory rows[i] against refs[i], as assert_oracle"""
    for i, (b, o) in enumerate(zip(rows, refs)):
        assert st[i] == o["status"] == 0, (label, b, st[i], o["status"])
        fig = backward_figures(K[b], k[b], dJ[i], o)
        print(f"{label} b={b}: {show(fig)}")
        assert all(v < RTOL for v in fig.values()), (label, b, fig)


# ---- the test bodies the files share --------------------------------------------------------------------------------------------------------
def check_gated_twin(leg):
    """The sweep under a lambda retry schedule (retry_problem): attempts and lambdas used are the reference loop's, some trajectory is
    swept more than once, and every trajectory's last sweep is the oracle's.  (The launch string has no token for the gated twin:
    that it ran is inferred from attempts > 1.)"""
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
    assert_backward_oracle(st, dJ, K, k, [r["out"] for r in refs], range(p["batch"]), f"gated {leg}")


def check_retry_outcomes_on_the_oracle():
    """(CPU) what check_gated_twin relies on: at the start lambdas some trajectories fail and some do not, exactly the failing ones
    are swept again, and every trajectory's last sweep succeeds"""
    for leg in RETRY:
        p, refs = retry_problem(leg), retry_reference(leg)
        first = [pipeline.run_trajectory(p, b, lam=float(p["lam0"][b]), pd_stride=RETRY_PD)["status"] for b in range(p["batch"])]
        assert any(s > 0 for s in first) and any(s == 0 for s in first), (leg, first)
        assert all(r["out"]["status"] == 0 for r in refs), (leg, [r["out"]["status"] for r in refs])
        assert [len(r["visited"]) > 1 for r in refs] == [s > 0 for s in first], leg


def check_listed_twin(p, refs, listed, rx_const, label):
    """backward_partial on the scattered list `listed` of problem p (refs: the oracle's runs of the whole batch)"""
    with fresh_engine(p) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=rx_const)
        st, dJ = e.backward_partial(listed, p["lam"])
        K, k = e.gains()
        lb = e.last_launch("backward")
    assert ":w1:" in lb and ":uni" in lb and lb.endswith(":subset") and ((":rxc" in lb) == rx_const), lb
    assert_backward_oracle(st, dJ, K, k, [refs[b] for b in listed], listed, label)


def check_uniform_against_general(label, task, T, min_N, dense, rx_const, **kw):
    """the uniform form against the general per-DoF-list form (KPILQR_FUSED_UNI=0) of the same sweep, key-point ordered payload"""
    uni = run(task, T, min_N, dense, "raw", rx_const, **kw)
    gen = run(task, T, min_N, dense, "raw", rx_const, general=True, **kw)
    assert_form(uni, "raw"); assert_form(gen, "raw", general=True)
    assert_forms_agree(uni, gen, label)
