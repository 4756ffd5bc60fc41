"""CPU tests of the boundary of the FP32 key-point column upload: kpilqr_upload_kp_columns_f32 / kpilqr_upload_kp_columns_f32_partial
exist in the header, the binding and the built library with the documented signatures, the header says what a caller has to know --
the ENCODING above all, which is the caller's side --, synth.kp_columns_f32 follows it, and the numpy restatement of the pipeline run
on the decoded columns stays inside the 1e-6 the gains are held to (tests/test_gpu_columns_f32.py runs the feature)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _columns_f32 as cf
import trajoptkp_amd
from oracle import crosscheck as cc
from trajoptkp_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kpilqr.h")).read()
FLAT = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S))       # declarations without their comments, on one line
SIGNATURES = {
    "kpilqr_upload_kp_columns_f32": "kpilqr_ctx *ctx, const float *columns32 , int entries",
    "kpilqr_upload_kp_columns_f32_partial": "kpilqr_ctx *ctx, int count, const int *traj, const float *columns32 , int entries",
}


def test_header_declares_both_calls():
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", FLAT)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args, (name, m.group(1))
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump


def test_binding_lists_both_symbols():
    assert set(SIGNATURES) <= set(_lib.SYMBOLS) and set(SIGNATURES) <= _lib.OPTIONAL_SYMBOLS
    par = inspect.signature(trajoptkp_amd.Engine.upload_kp_columns_f32).parameters
    assert list(par) == ["self", "columns32", "traj"] and par["traj"].default is None
    assert "f32" not in "".join(inspect.signature(synth.upload).parameters)      # synth.upload gains no new default


def test_library_exports_them_and_refuses_null_arguments():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in SIGNATURES:
        assert hasattr(L, name) and re.search(r"\bT " + name + r"\b", out), name
    assert L.kpilqr_upload_kp_columns_f32(None, None, 0) == _lib.ERR_ARG
    assert L.kpilqr_upload_kp_columns_f32_partial(None, 0, None, None, 0) == _lib.ERR_ARG
    assert L.kpilqr_upload_kp_columns_f32_partial(None, 1, None, None, 0) == _lib.ERR_ARG


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("exactly those of kpilqr_upload_kp_columns / kpilqr_upload_kp_columns_partial",
                 "kind-2 slots of DoFs >= num_ctrl are present and ignored",
                 "before anything is enqueued or the context changes", "a view never allocates",
                 # the encoding: the caller's side
                 "Encoding (the CALLER's side)", "the unit entry is REMOVED before the cast -- the subtraction in double",
                 "columns32[e][0][r] = (float)(A(r, d) - (r == d ? 1 : 0))",
                 "columns32[e][1][r] = (float)(A(r, d + dof) - (r == d + dof ? 1 : 0))",
                 "columns32[e][2][r] = (float) B(r, d)",
                 # the decoding: the library's side
                 "Decoding (the LIBRARY's side)", "an exact widening, followed by ONE IEEE addition of 1.0 at the unit row of kinds 0 and 1",
                 "and nowhere else", "FP32 subnormals widen exactly", "NaN stays NaN", "+-inf stays +-inf",
                 "bit for bit, what kpilqr_upload_kp_columns would hold if it were given those decoded doubles",
                 "nothing downstream knows the difference",
                 "ONE hipMemcpyAsync of the floats into a staging buffer the context owns", "ONE launch of a streaming kernel",
                 "Memory cost: the staging buffer, entries*3n*4 bytes", "KPILQR_ERR_ALLOC",
                 # out of scope
                 "Out of scope: the chunk pipeline (kpilqr_stream_io and kpilqr_stream_io2 are fixed structs",
                 "FP32 for the x+ / x- payloads, residuals, residual Jacobians, nominal controls, or inside any sweep",
                 "the batch shim", "an environment switch", "detect the calls by their symbols"):
        assert word in doc, word


def test_no_new_environment_switch():
    csrc = os.path.join(ROOT, "trajoptkp_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")))
    read = set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src))
    assert not [n for n in read if "F32" in n or "COL" in n], read
    assert "getenv" not in open(os.path.join(csrc, "columns_f32.hip")).read()


# ---- the encoding --------------------------------------------------------------------------------------------------------------------
GOLDEN_T37 = dict(task="panda_reaching", T=37, batch=2, min_N=5)
SHAPES = dict(cc.GOLDEN, panda_T37=GOLDEN_T37, hopper_T50=dict(task="hopper", T=50, batch=2, min_N=5))
LAMS = (1e-4, 0.1, 10.0)


@pytest.fixture(scope="module", params=sorted(SHAPES))
def case(request):
    p = synth.make_problem(**SHAPES[request.param])
    cols = synth.kp_columns(p)
    dofs = synth.kp_entry_dofs(p)
    return dict(name=request.param, p=p, cols=cols, dofs=dofs, dec=synth.decode_kp_columns_f32(synth.kp_columns_f32(p), dofs, p["dof"]))


def test_synth_helper_follows_the_header(case):
    """synth.kp_columns_f32 decoded (astype(float64), + 1.0 at the unit rows) against the FP64 columns: at most 2^-24 relative per
    element of A - I and of B -- the round-to-nearest-even cast of a value in FP32's normal range -- plus the two roundings the unit
    rows see in double (the subtraction and the one addition of 1.0: 2^-53 of a value near 1 each, 2^-52 together)."""
    p, cols, dofs, dec = case["p"], case["cols"], case["dofs"], case["dec"]
    c32 = synth.kp_columns_f32(p)
    assert c32.dtype == np.float32 and c32.shape == cols.shape == (len(dofs), 3, p["n"])
    e = np.arange(len(dofs))
    unit = np.zeros_like(cols)
    unit[e, 0, dofs] = 1.0; unit[e, 1, dofs + p["dof"]] = 1.0
    resid = cols - unit                                   # A - I and B: what the floats carry
    assert np.max(np.abs(resid)) < 0.5                    # (the stand-in dynamics: a column of A is a unit vector plus O(dt))
    assert np.array_equal(c32, resid.astype(np.float32))  # the header's formula, the subtraction in double
    normal = np.abs(resid) >= np.finfo(np.float32).tiny
    assert np.all(resid[~normal] == 0.0)                  # (nothing of these inputs falls into FP32's subnormal range)
    bound = 2.0 ** -24 * np.abs(resid) + 2.0 ** -52 * unit
    assert np.all(np.abs(dec - cols) <= bound)
    assert np.count_nonzero(dec != cols) > cols.size // 4  # ... and it IS a rounding: most non-zero elements move


def test_decoded_columns_keep_the_results_inside_the_bar(case):
    """np_interp -> np_backward -> np_forward of oracle/crosscheck.py on the decoded columns against the same on the unrounded ones:
    K, k and U differ (the rounding reaches them) and each stays below 1e-6, the bar include/kpilqr.h names for the gains."""
    p, cols, dec = case["p"], case["cols"], case["dec"]
    alphas = (np.arange(1, 7) / 6.0) ** 2
    for b in range(p["batch"]):
        A0, B0 = cf.columns_to_AB(p, cols, b)
        fdA, fdB = cc.np_fd(p, b)
        assert np.array_equal(A0, fdA) and np.array_equal(B0, fdB)          # the FP64 columns ARE what np_fd differences
        A1, B1 = cf.columns_to_AB(p, dec, b)
        assert np.count_nonzero(A1 != A0) >= 100
        l = cc.np_cost(p, b)
        for lam in LAMS:
            out = []
            for A, B in ((A0, B0), (A1, B1)):
                Ai, Bi = cc.np_interp(p, b, A, B)
                st, K, k, _ = cc.np_backward(Ai, Bi, *l, lam)
                assert st == 0
                _, U = cc.np_forward(Ai, Bi, K, k, *l, p["u_nom"][b], p["ctrl_lim"], alphas)
                out.append(dict(K=K, k=k, U=U))
            for key in ("K", "k", "U"):
                err = cc.rel(out[1][key], out[0][key])
                print(f"{case['name']} b={b} lambda={lam:g} {key}: {err:.2e}")
                assert 0.0 < err < 1e-6, (case["name"], b, lam, key, err)
