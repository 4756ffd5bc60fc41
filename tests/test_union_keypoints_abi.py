"""CPU tests of the boundary of KPILQR_FLAG_UNION_KEYPOINTS: the flag and the two hooks exist in the header, the binding and the
built library, and the header says what a caller has to know (tests/test_gpu_union_keypoints.py runs the feature)."""
import os
import re
import subprocess

import trajoptkp_amd
from trajoptkp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kpilqr.h")).read()
HOOKS = ("kpilqr_get_union_keypoints", "kpilqr_get_union_columns")


def test_binding_exposes_the_flag():
    assert _lib.FLAG_UNION_KEYPOINTS == 8
    assert re.search(r"#define\s+KPILQR_FLAG_UNION_KEYPOINTS\s+8\b", HEADER)
    for other in (_lib.FLAG_GENERIC_KERNELS, _lib.FLAG_TILED_KERNELS, _lib.FLAG_FUSED):
        assert other & _lib.FLAG_UNION_KEYPOINTS == 0
    assert set(HOOKS) <= set(_lib.SYMBOLS) and set(HOOKS) <= _lib.OPTIONAL_SYMBOLS      # detected by symbol: no version bump
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)


def test_library_exports_the_hooks():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in HOOKS:
        assert hasattr(L, name) and re.search(r"\bT " + name + r"\b", out), name
        assert re.search(r"\bint\s+" + name + r"\s*\(kpilqr_ctx \*", HEADER), name
    # a NULL context is refused before anything touches a device
    assert L.kpilqr_get_union_keypoints(None, None, None, 0) == _lib.ERR_ARG
    assert L.kpilqr_get_union_columns(None, None, 0) == _lib.ERR_ARG


def test_engine_takes_the_keyword():
    import inspect
    sig = inspect.signature(trajoptkp_amd.Engine.__init__)
    assert sig.parameters["union_keypoints"].default is False
    assert callable(trajoptkp_amd.Engine.get_union_keypoints) and callable(trajoptkp_amd.Engine.get_union_columns)


def test_header_documents_the_route():
    doc = re.sub(r"\s+", " ", HEADER)
    for word in ("KPILQR_FLAG_UNION_KEYPOINTS", ":union", '"kp_union"', "kpilqr_get_union_keypoints", "kpilqr_get_union_columns",
                 "1e-16", "per key-point change", "kpilqr_iterate_streamed ignore"):
        assert word in doc, word


def test_no_new_environment_switch():
    """The flag is a context flag: the library reads no KPILQR_* environment variable for it (tests/test_abi.py holds every switch
    the library does read to the header's list)."""
    src = ""
    for f in sorted(os.listdir(os.path.join(ROOT, "trajoptkp_amd", "csrc"))):
        if f.endswith((".cpp", ".hip", ".h")):
            src += open(os.path.join(ROOT, "trajoptkp_amd", "csrc", f)).read()
    read = set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src))
    assert read and not [n for n in read if "UNION" in n], read
    assert "getenv" not in open(os.path.join(ROOT, "trajoptkp_amd", "csrc", "kp_union.hip")).read()
