"""CPU tests of the boundary of the second half of partial re-linearisation -- residuals, nominal controls and step records of a
subset: the four entry points exist in the header, the binding and the built library with the documented signatures, and the header
says what a caller has to know (tests/test_gpu_partial_inputs.py runs the feature)."""
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
    "kpilqr_upload_residuals_partial": "kpilqr_ctx *ctx, int count, const int *traj, const double *r, const double *r_x, const double *r_u",
    "kpilqr_upload_nominal_partial": "kpilqr_ctx *ctx, int count, const int *traj, const double *u_nom",
    "kpilqr_fd_interpolate_partial": "kpilqr_ctx *ctx, int count, const int *traj",
    "kpilqr_cost_derivs_partial": "kpilqr_ctx *ctx, int count, const int *traj",
}


def test_header_declares_the_four_entry_points():
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", FLAT)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args, (name, m.group(1))
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump


def test_binding_lists_them_as_optional_symbols():
    assert set(SIGNATURES) <= set(_lib.SYMBOLS) and set(SIGNATURES) <= _lib.OPTIONAL_SYMBOLS
    for name in ("upload_residuals_partial", "upload_nominal_partial", "fd_interpolate_partial", "cost_derivs_partial"):
        assert callable(getattr(trajoptkp_amd.Engine, name)), name
    import inspect
    par = inspect.signature(trajoptkp_amd.Engine.upload_residuals_partial).parameters
    assert list(par) == ["self", "traj", "r", "r_x", "r_u"] and all(par[k].default is None for k in ("r", "r_x", "r_u"))


def test_library_exports_them_and_refuses_a_null_context():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in SIGNATURES:
        assert hasattr(L, name) and re.search(r"\bT " + name + r"\b", out), name
    # a NULL context is refused before anything touches a device
    assert L.kpilqr_upload_residuals_partial(None, 0, None, None, None, None) == _lib.ERR_ARG
    assert L.kpilqr_upload_nominal_partial(None, 0, None, None) == _lib.ERR_ARG
    assert L.kpilqr_fd_interpolate_partial(None, 0, None) == _lib.ERR_ARG
    assert L.kpilqr_cost_derivs_partial(None, 0, None) == _lib.ERR_ARG


def test_host_library_exports_the_counters():
    host_lib = os.path.join(os.path.dirname(_lib.LIB_PATH), "libkpilqr_host.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", host_lib], text=True)
    for name in ("kpilqr_host_run_acrobot_batch3", "kpilqr_host_run_acrobot_batch4"):
        assert re.search(r"\bT " + name + r"\b", out), name


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("strictly increasing and within [0, batch)", "count = 0 is a no-op returning KPILQR_OK", "COMPACT",
                 "one hipMemcpyAsync per array and run of adjacent trajectories", "no staging buffer, no scatter kernel",
                 "names the whole-batch call to make first", "in constant-Jacobian mode", "before a whole r_x has been uploaded",
                 "before a whole r_u upload or broadcast", "r has no precondition", "all T+1 rows finite",
                 "no byte of any other trajectory's records is written", "hold a complete linearisation from an earlier whole or partial call",
                 "ONE launch per stage", "only when `traj` is pageable", "RESIDENT jobs", "KPILQR_FD_INTERP=0",
                 "while ranges are pending after kpilqr_update_keypoints", "On a KPILQR_FLAG_FUSED context both return KPILQR_ERR_STATE",
                 "fd_kp_interpolate:subset", "kp_columns_interpolate:subset", "fd_difference+interpolate:subset",
                 "Out of scope: the sweeps still run over the whole batch"):
        assert word in doc, word


def test_no_new_environment_switch():
    """The calls a host makes choose the route: the library reads no KPILQR_* environment variable for it (tests/test_abi.py holds
    every switch the library does read to the header's list)."""
    csrc = os.path.join(ROOT, "trajoptkp_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")))
    read = set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src))
    listed = set(re.findall(r"^ \*   (KPILQR_[A-Z0-9_]+) ", HEADER, flags=re.M))
    assert read and read <= listed, read - listed
    assert not [n for n in read if "PARTIAL" in n or "SUBSET" in n or "WHOLE" in n], read
    assert src.count("getenv(") == 1            # env_int, called from read_tuning_from_env alone
    assert len(re.findall(r'env_int\("', src)) == 11      # the eleven switches of Ctx::Tuning, as before
