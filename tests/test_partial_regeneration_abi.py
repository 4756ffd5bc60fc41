"""CPU tests of the boundary of partial re-linearisation: the four entry points exist in the header, the binding and the built
library with the documented signatures, and the header says what a caller has to know
(tests/test_gpu_partial_regeneration.py runs the feature)."""
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
    "kpilqr_update_keypoints": "kpilqr_ctx *ctx, int count, const int *traj, const int *kp_offsets , const int *kp_times",
    "kpilqr_upload_fd_kp_partial": "kpilqr_ctx *ctx, int count, const int *traj, const void *slab, int entries, double eps",
    "kpilqr_upload_kp_columns_partial": "kpilqr_ctx *ctx, int count, const int *traj, const double *columns, int entries",
    "kpilqr_download_gains_partial": "kpilqr_ctx *ctx, int count, const int *traj, double *K , double *k",
}


def test_header_declares_the_four_entry_points():
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", FLAT)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args, (name, m.group(1))
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump


def test_binding_lists_them_as_optional_symbols():
    assert set(SIGNATURES) <= set(_lib.SYMBOLS) and set(SIGNATURES) <= _lib.OPTIONAL_SYMBOLS
    for name in ("update_keypoints_rows", "upload_fd_kp_partial", "upload_kp_columns_partial", "gains"):
        assert callable(getattr(trajoptkp_amd.Engine, name)), name
    import inspect
    assert inspect.signature(trajoptkp_amd.Engine.gains).parameters["traj"].default is None


def test_library_exports_them_and_refuses_a_null_context():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in SIGNATURES:
        assert hasattr(L, name) and re.search(r"\bT " + name + r"\b", out), name
    # a NULL context is refused before anything touches a device
    assert L.kpilqr_update_keypoints(None, 0, None, None, None) == _lib.ERR_ARG
    assert L.kpilqr_upload_fd_kp_partial(None, 0, None, None, 0, 1e-6) == _lib.ERR_ARG
    assert L.kpilqr_upload_kp_columns_partial(None, 0, None, None, 0) == _lib.ERR_ARG
    assert L.kpilqr_download_gains_partial(None, 0, None, None, None) == _lib.ERR_ARG


def test_header_documents_the_route():
    doc = re.sub(r"\s+", " ", HEADER)
    for word in ("PENDING", "KPILQR_ERR_STATE and names what is missing", "DOUBLED", "5.9 GB", "eps must match", "a context has one eps",
                 "strictly increasing", "WAITS for the stream", "count = 0 is a no-op", "Out of scope", "kp_partial.hip"):
        assert word in doc, word


def test_no_new_environment_switch():
    """The route is chosen by the calls a host makes: the library reads no KPILQR_* environment variable for it (tests/test_abi.py
    holds every switch the library does read to the header's list)."""
    csrc = os.path.join(ROOT, "trajoptkp_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")))
    read = set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src))
    listed = set(re.findall(r"^ \*   (KPILQR_[A-Z0-9_]+) ", HEADER, flags=re.M))
    assert read and read <= listed, read - listed
    assert not [n for n in read if "PARTIAL" in n or "UPDATE" in n or "RELOC" in n], read
    for f in ("kp_partial.hip", "kp_merge.h"):
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f
    assert "kp_partial.o" in open(os.path.join(csrc, "Makefile")).read()
