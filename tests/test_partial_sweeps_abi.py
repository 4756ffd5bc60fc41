"""CPU tests of the boundary of the sweeps over a listed subset of the batch: the three entry points exist in the header, the binding
and the built library with the documented signatures, a NULL context is refused, and the header says what a caller has to know
(tests/test_gpu_partial_sweeps.py runs the feature)."""
import inspect
import os
import re
import subprocess

import trajoptkp_amd
from trajoptkp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kpilqr.h")).read()
FLAT = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)           # declarations without their comments ...
FLAT = re.sub(r"\s+", " ", FLAT)                               # ... on one line
SIGNATURES = {
    "kpilqr_backward_partial": "kpilqr_ctx *ctx, int count, const int *traj, const double *lambda , int pd_check_stride, int *status , double *delta_J",
    "kpilqr_forward_linear_partial": "kpilqr_ctx *ctx, int count, const int *traj, const double *alphas, double *cost_pred , double *U_alpha",
    "kpilqr_iterate_partial": "kpilqr_ctx *ctx, int count, const int *traj, const double *lambda , int pd_check_stride, const double *alphas",
}


def test_header_declares_the_three_entry_points():
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", FLAT)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args, (name, m.group(1))
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump


def test_binding_lists_them_as_optional_symbols():
    assert set(SIGNATURES) <= set(_lib.SYMBOLS) and set(SIGNATURES) <= _lib.OPTIONAL_SYMBOLS
    for name in ("backward_partial", "forward_linear_partial", "iterate_partial"):
        assert callable(getattr(trajoptkp_amd.Engine, name)), name
    par = inspect.signature(trajoptkp_amd.Engine.backward_partial).parameters
    assert list(par)[:3] == ["self", "traj", "lam"] and par["lam"].default is None


def test_library_exports_them_and_refuses_a_null_context():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in SIGNATURES:
        assert hasattr(L, name) and re.search(r"\bT " + name + r"\b", out), name
    # a NULL context is refused before anything touches a device
    assert L.kpilqr_backward_partial(None, 0, None, None, 100, None, None) == _lib.ERR_ARG
    assert L.kpilqr_forward_linear_partial(None, 0, None, None, None, None) == _lib.ERR_ARG
    assert L.kpilqr_iterate_partial(None, 0, None, None, 100, None) == _lib.ERR_ARG


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("Sweeps of a subset", "strictly increasing and within [0, batch)", "count = 0 is a no-op returning KPILQR_OK",
                 # the compact layouts
                 "Host arrays are COMPACT: the listed trajectories' rows back to back in `traj` order",
                 "lambda [count]", "status [count]", "delta_J [count]", "cost_pred [count][n_alpha]", "U_alpha [count][n_alpha][T][m]",
                 # what a listed trajectory gets and what nobody else loses
                 "bit for bit what a context holding exactly the listed trajectories",
                 "No byte of an unlisted trajectory is written",
                 # the fused column-store rule
                 "a subset sweep reads the column store and never differences inside the sweep",
                 "differenced for the WHOLE batch first", "KPILQR_FLAG_UNION_KEYPOINTS is ignored",
                 "while ranges are pending after kpilqr_update_keypoints",
                 # form, retry, cost, scope
                 "What only arranges waves follows `count`", '":subset" appended last', "an unlisted trajectory is never armed",
                 "kpilqr_download_lambda_retry stays a whole-batch read", "A context that never makes these calls allocates and launches nothing for them",
                 "Out of scope: the chunk pipeline", "kpilqr_allreduce_linesearch sums whatever cost_pred and status are resident",
                 "only when `traj` is pageable"):
        assert word in doc, word
    # a "(since: ...)" note under the older sentences that said the sweeps cover the whole batch
    assert doc.count('(since: ') >= 4 and "Out of scope: the sweeps still run over the whole batch" in doc
