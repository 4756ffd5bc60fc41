"""CPU tests of the boundary of KPILQR_FLAG_EMBED_SHAPE: the flag and kpilqr_get_carrier_dims exist in the header, the binding and
the built library; the header's paragraph names the contract, the lambda rule and every call the library refuses on an embedded
context; the sweep kernels know nothing of it (tests/test_gpu_embed.py runs the feature)."""
import inspect
import os
import re
import subprocess

import trajoptkp_amd
from trajoptkp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trajoptkp_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "kpilqr.h")).read()
API = open(os.path.join(CSRC, "kpilqr_api.cpp")).read()


def _paragraph():
    """The comment at the flag's #define, white space collapsed."""
    m = re.search(r"#define\s+KPILQR_FLAG_EMBED_SHAPE\s+16\s*/\*(.*?)\*/", HEADER, re.S)
    assert m, "include/kpilqr.h does not define KPILQR_FLAG_EMBED_SHAPE as 16 with its paragraph"
    return re.sub(r"\s+", " ", m.group(1))


def test_binding_exposes_the_flag():
    assert _lib.FLAG_EMBED_SHAPE == 16
    assert re.search(r"#define\s+KPILQR_FLAG_EMBED_SHAPE\s+16\b", HEADER)
    for other in (_lib.FLAG_GENERIC_KERNELS, _lib.FLAG_TILED_KERNELS, _lib.FLAG_FUSED, _lib.FLAG_UNION_KEYPOINTS):
        assert other & _lib.FLAG_EMBED_SHAPE == 0
    assert "kpilqr_get_carrier_dims" in _lib.SYMBOLS and "kpilqr_get_carrier_dims" in _lib.OPTIONAL_SYMBOLS
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)                   # detected by symbol: no version bump


def test_library_exports_get_carrier_dims():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert hasattr(L, "kpilqr_get_carrier_dims") and re.search(r"\bT kpilqr_get_carrier_dims\b", out)
    assert re.search(r"\bint\s+kpilqr_get_carrier_dims\s*\(kpilqr_ctx \*ctx, kpilqr_dims \*out\)", HEADER)
    # a NULL context or output is refused before anything touches a device
    assert L.kpilqr_get_carrier_dims(None, None) == _lib.ERR_ARG
    d = _lib.Dims()
    import ctypes as C
    assert L.kpilqr_get_carrier_dims(None, C.byref(d)) == _lib.ERR_ARG


def test_engine_takes_the_keyword():
    sig = inspect.signature(trajoptkp_amd.Engine.__init__)
    assert sig.parameters["embed"].default is False
    assert callable(trajoptkp_amd.Engine.carrier_dims)


def test_header_names_every_refused_call():
    refused = re.findall(r'KP_NOT_EMBEDDED\(c, "(kpilqr_[a-z0-9_]+)"\)', API)
    assert len(refused) >= 40 and len(set(refused)) == len(refused)
    doc = _paragraph()
    scope = doc[doc.index("Out of scope"):]
    missing = [name for name in refused if not re.search(r"\b" + name + r"\b", scope)]
    assert not missing, missing
    assert "kpilqr_device_ptr of a shape-dependent buffer" in scope and "KPILQR_ERR_STATE" in scope
    assert "not on an embedded context" in scope and "not on an embedded context" in API
    # every declared entry point is either refused or named as in scope in front of that list
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*\*?\s*(kpilqr_[a-z0-9_]+)\s*\(", HEADER, re.M))
    head = doc[:doc.index("Out of scope")]
    free = {"kpilqr_create", "kpilqr_destroy", "kpilqr_version", "kpilqr_backward_variant", "kpilqr_forward_variant"}
    unnamed = [n for n in sorted(declared - set(refused) - free)
               if not re.search(r"\b" + re.sub(r"_(alloc|unique_id|init)$", "", n), head)]
    assert not unnamed, unnamed


def test_header_documents_contract_and_lambda_rule():
    doc = _paragraph()
    for word in ("KPILQR_FLAG_FUSED", "carrier", "smallest n'", "dof <= dof'", "m <= dof", "copies of the trajectory's list 0",
                 "kpilqr_get_carrier_dims", ":emb14x7", "(-1, 1)", "lambda I", "KPILQR_ERR_ARG", "lambda = NULL", "m' == m",
                 "Costs", "profiles/embedded_shapes.txt", "No environment switch", "KPILQR_VERSION is unchanged"):
        assert word in doc, word


def test_sweep_kernels_do_not_see_the_embedding():
    """The embed struct is consulted at the ABI boundary alone: kpilqr_api.cpp and embed.hip."""
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".cpp")) and f not in ("kpilqr_api.cpp", "embed.hip"):
            src = open(os.path.join(CSRC, f)).read()
            assert "embed" not in src and "emb_" not in src, f
    assert "getenv" not in open(os.path.join(CSRC, "embed.hip")).read()
    read = set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', API))
    assert read and not [n for n in read if "EMBED" in n], read
