"""CPU tests of the boundary of the FP32 gain download: kpilqr_download_gains_f32 / kpilqr_download_gains_f32_partial exist in the
header, the binding and the built library with the documented signatures, refuse a NULL context before anything touches a device,
and the header says what a caller has to know (tests/test_gpu_gains_f32.py runs the feature)."""
import inspect
import os
import re
import subprocess

import trajoptkp_amd
from trajoptkp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kpilqr.h")).read()
FLAT = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S))       # declarations without their comments, on one line
SIGNATURES = {
    "kpilqr_download_gains_f32": "kpilqr_ctx *ctx, float *K32 , double *k",
    "kpilqr_download_gains_f32_partial": "kpilqr_ctx *ctx, int count, const int *traj, float *K32 , double *k",
}


def test_header_declares_both_calls():
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", FLAT)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args, (name, m.group(1))
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump


def test_binding_lists_both_symbols():
    assert set(SIGNATURES) <= set(_lib.SYMBOLS) and set(SIGNATURES) <= _lib.OPTIONAL_SYMBOLS
    par = inspect.signature(trajoptkp_amd.Engine.gains).parameters
    assert list(par) == ["self", "traj", "want_K", "want_k", "f32"] and par["f32"].default is False      # the default stays FP64


def test_library_exports_them_and_refuses_a_null_context():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in SIGNATURES:
        assert hasattr(L, name) and re.search(r"\bT " + name + r"\b", out), name
    assert L.kpilqr_download_gains_f32(None, None, None) == _lib.ERR_ARG
    assert L.kpilqr_download_gains_f32_partial(None, 0, None, None, None) == _lib.ERR_ARG
    assert L.kpilqr_download_gains_f32_partial(None, 1, None, None, None) == _lib.ERR_ARG


def test_host_library_exports_the_new_runner_and_keeps_the_old():
    host_lib = os.path.join(os.path.dirname(_lib.LIB_PATH), "libkpilqr_host.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", host_lib], text=True)
    for name in ("kpilqr_host_run_acrobot_batch4", "kpilqr_host_run_acrobot_batch5"):
        assert re.search(r"\bT " + name + r"\b", out), name


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("exactly those of kpilqr_download_gains / kpilqr_download_gains_partial",
                 "strictly increasing and within [0, batch), else KPILQR_ERR_ARG and nothing is enqueued",
                 "either pointer may be NULL", "a NULL context is KPILQR_ERR_ARG", "a view never allocates",
                 "IEEE round-to-nearest-even", "what the C cast (float) gives", "produced, not flushed", "become +-inf", "NaN stays NaN",
                 "k stays FP64", "The resident FP64 K is never written", "ONE launch", "ONE hipMemcpyAsync",
                 "Memory cost: the float buffer, count*T*n*m*4 bytes", "KPILQR_ERR_ALLOC",
                 "Out of scope: kpilqr_iterate_streamed", "detect the calls by their symbols"):
        assert word in doc, word


def test_no_new_environment_switch():
    csrc = os.path.join(ROOT, "trajoptkp_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")))
    read = set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src))
    assert not [n for n in read if "F32" in n or "GAIN" in n], read
    assert "getenv" not in open(os.path.join(csrc, "gains.hip")).read()
