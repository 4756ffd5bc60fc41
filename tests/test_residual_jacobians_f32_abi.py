"""CPU tests of the boundary of the FP32 residual-Jacobian upload: kpilqr_upload_residual_jacobians_f32 /
kpilqr_upload_residual_jacobians_f32_partial exist in the header, the binding and the built library with the documented signatures,
the header says what a caller has to know, synth.residual_jacobians_f32 is the plain cast, and the numpy restatement of the pipeline
run on the decoded Jacobians stays inside the 1e-6 the gains are held to (tests/test_gpu_residual_jacobians_f32.py runs the feature)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _residual_jacobians_f32 as rj
import trajoptkp_amd
from oracle import crosscheck as cc
from trajoptkp_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kpilqr.h")).read()
FLAT = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S))       # declarations without their comments, on one line
SIGNATURES = {
    "kpilqr_upload_residual_jacobians_f32": "kpilqr_ctx *ctx, const float *r_x32 , const float *r_u32",
    "kpilqr_upload_residual_jacobians_f32_partial": "kpilqr_ctx *ctx, int count, const int *traj, const float *r_x32 , const float *r_u32",
}


# ---- 1. the header -----------------------------------------------------------------------------------------------------------------
def test_header_declares_both_calls():
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", FLAT)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args, (name, m.group(1))
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    doc = doc[doc.index("The per-step residual Jacobians as FP32"):]
    doc = doc[:doc.index("int kpilqr_upload_residual_jacobians_f32(")]
    for word in (# the equivalence to the FP64 calls
                 "bit for bit and flag for flag, what kpilqr_upload_residuals(ctx, NULL, rx, ru, NULL, NULL)",
                 "kpilqr_upload_residuals_partial(ctx, count, traj, NULL, rx, ru)",
                 "rx[i] = (double)r_x32[i] and ru[i] = (double)r_u32[i]",
                 "the end of constant-Jacobian mode", "kpilqr_last_launch (:ru0, :rxc)", "nothing downstream knows the difference",
                 "r is small and stays FP64", "Both pointers NULL is KPILQR_OK with nothing enqueued",
                 # exact widening
                 "A plain (float) cast", "an exact widening and nothing else", "FP32 subnormals widen to their value", "+-inf stays +-inf",
                 "-0 stays -0", "NaN stays NaN",
                 # the three refusals, the view and the embedded refusal
                 "each before anything is enqueued or changed", "the three refusals of kpilqr_upload_residuals_partial",
                 "while the context holds constant residual Jacobians", "of a subset before a whole r_x",
                 "on a context that runs without control residuals", "a view never allocates", "not on an embedded context",
                 # the staging memory
                 "Memory cost: the staging buffer, 4 bytes x (elements of r_x32 + r_u32)", "3.5 MB per trajectory at the headline shape",
                 "freed by kpilqr_destroy", "KPILQR_ERR_ALLOC when it cannot be had: the context is unchanged",
                 "ONE hipMemcpyAsync per array", "no copy per run of a scattered list",
                 # what the bar holds for
                 "the 1e-6 bar the gains are held to is held for K and k", "NOT promised for the clamped controls",
                 # out of scope
                 "inside the chunks of kpilqr_iterate_streamed*", "embedded contexts; r itself; a bounded staging arena",
                 "an environment switch", "KPILQR_VERSION is unchanged", "detect the calls by their symbols"):
        assert word in doc, word


def test_no_new_environment_switch():
    csrc = os.path.join(ROOT, "trajoptkp_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")))
    read = set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src))
    assert not [n for n in read if "F32" in n or "RES" in n or "JAC" in n], read
    assert "getenv" not in open(os.path.join(csrc, "residuals_f32.hip")).read()


# ---- 2. the binding and the library ------------------------------------------------------------------------------------------------
def test_binding_lists_both_symbols():
    assert set(SIGNATURES) <= set(_lib.SYMBOLS) and set(SIGNATURES) <= _lib.OPTIONAL_SYMBOLS
    par = inspect.signature(trajoptkp_amd.Engine.upload_residual_jacobians_f32).parameters
    assert list(par) == ["self", "r_x32", "r_u32", "traj"] and all(par[k].default is None for k in ("r_x32", "r_u32", "traj"))
    assert "f32" not in "".join(inspect.signature(synth.upload).parameters)      # synth.upload gains no new default


def test_library_exports_them_and_refuses_a_null_context():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in SIGNATURES:
        assert hasattr(L, name) and re.search(r"\bT " + name + r"\b", out), name
    assert L.kpilqr_upload_residual_jacobians_f32(None, None, None) == _lib.ERR_ARG
    assert L.kpilqr_upload_residual_jacobians_f32_partial(None, 0, None, None, None) == _lib.ERR_ARG
    assert L.kpilqr_upload_residual_jacobians_f32_partial(None, 1, None, None, None) == _lib.ERR_ARG


# ---- 3. / 4. the cast and what it costs ------------------------------------------------------------------------------------------------
SHAPES = dict(cc.GOLDEN, panda_T37=dict(task="panda_reaching", T=37, batch=2, min_N=5), acrobot_T50=dict(task="acrobot", T=50, batch=2, min_N=5))
LAMS = (1e-4, 0.1, 10.0)
CASES = [(name, dense) for name in sorted(SHAPES) for dense in (True, "smooth")]


@pytest.fixture(scope="module", params=CASES, ids=[f"{n}-{'dense' if d is True else d}" for n, d in CASES])
def case(request):
    name, dense = request.param
    p = synth.make_problem(**dict(SHAPES[name], dense_residuals=dense))
    return dict(name=f"{name}-{dense}", p=p, q=rj.decoded_twin(p))


def test_synth_helper_is_the_plain_cast_and_it_is_a_rounding(case):
    """synth.residual_jacobians_f32 is astype(float32); widened back it stays within 2^-24 relative of the original -- the
    round-to-nearest-even cast of a value in FP32's normal range -- and at least half of the non-zero elements move."""
    p, q = case["p"], case["q"]
    x32, u32 = synth.residual_jacobians_f32(p)
    assert x32.dtype == u32.dtype == np.float32 and x32.shape == p["r_x"].shape and u32.shape == p["r_u"].shape
    assert np.array_equal(x32, rj.cast(p["r_x"])) and np.array_equal(u32, rj.cast(p["r_u"]))
    assert np.array_equal(rj.decode(x32), q["r_x"]) and np.array_equal(rj.decode(u32), q["r_u"])
    for key in ("r_x", "r_u"):
        a, d = p[key], q[key]
        nz = a != 0.0
        assert np.all(np.abs(a[nz]) >= np.finfo(np.float32).tiny)       # (nothing of these inputs falls into FP32's subnormal range)
        assert np.all(np.abs(d - a) <= 2.0 ** -24 * np.abs(a))
        assert 2 * np.count_nonzero(d != a) >= np.count_nonzero(nz), key
    assert np.count_nonzero(p["r_x"]) > 0


def test_decoded_jacobians_keep_the_results_inside_the_bar(case):
    """np_cost -> np_backward -> np_forward of oracle/crosscheck.py on the decoded Jacobians against the same on the unrounded ones:
    K, k and U differ (the rounding reaches them) and each stays below 1e-6, the bar include/kpilqr.h names for the gains.
    (Hopper, whose l_xx is rank-deficient, is not among the inputs: its clamped controls leave the bar, as the header says.)"""
    p, q = case["p"], case["q"]
    alphas = (np.arange(1, 7) / 6.0) ** 2
    for b in range(p["batch"]):
        Ai, Bi = cc.np_interp(p, b, *cc.np_fd(p, b))
        for lam in LAMS:
            out = []
            for prob in (p, q):
                l = cc.np_cost(prob, b)
                st, K, k, _ = cc.np_backward(Ai, Bi, *l, lam)
                assert st == 0
                _, U = cc.np_forward(Ai, Bi, K, k, *l, p["u_nom"][b], p["ctrl_lim"], alphas)
                out.append(dict(K=K, k=k, U=U))
            for key in ("K", "k", "U"):
                err = cc.rel(out[1][key], out[0][key])
                print(f"{case['name']} b={b} lambda={lam:g} {key}: {err:.2e}")
                assert 0.0 < err < 1e-6, (case["name"], b, lam, key, err)
