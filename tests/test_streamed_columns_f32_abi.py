"""CPU tests of the boundary of kpilqr_iterate_streamed3 (the chunk pipeline taking the key-point columns as ENCODED FP32): the struct
and the call exist in the header, the binding and the built library, the ctypes structure has the C compiler's layout, a NULL context
or struct is refused before anything touches a device, and the header says what a caller has to know
(tests/test_gpu_streamed_columns_f32.py runs the feature)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import trajoptkp_amd
from trajoptkp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kpilqr.h")).read()
FLAT = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S))       # declarations without their comments, on one line
NAME = "kpilqr_iterate_streamed3"
FIELDS = ["struct_size", "io2", "kp_columns32"]
OLD_PARAMETERS = ["self", "fd", "fd_kp", "kp_cols", "eps", "r", "r_x", "r_u", "u_nom", "lam", "K", "k", "cost_pred", "delta_J", "status",
                  "pd_stride", "nchunks", "K32", "gain_traj"]


def test_header_declares_the_struct_and_the_call():
    m = re.search(r"typedef struct \{([^{}]*)\} kpilqr_stream_io3;", FLAT)
    assert m, "kpilqr_stream_io3"
    members = [re.sub(r"\s+", " ", x).strip() for x in m.group(1).split(";") if x.strip()]
    assert members == ["size_t struct_size", "kpilqr_stream_io2 io2", "const float *kp_columns32"], members
    m = re.search(r"\bint " + NAME + r"\(([^)]*)\)", FLAT)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "kpilqr_ctx *ctx, const kpilqr_stream_io3 *io3, int pd_check_stride, int nchunks"
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump
    assert trajoptkp_amd.load().kpilqr_version() == 410


def test_binding_lists_the_symbol_and_keeps_the_old_parameters():
    assert NAME in _lib.SYMBOLS and NAME in _lib.OPTIONAL_SYMBOLS
    par = inspect.signature(trajoptkp_amd.Engine.iterate_streamed).parameters
    assert list(par) == OLD_PARAMETERS
    new = inspect.signature(trajoptkp_amd.Engine.iterate_streamed3).parameters
    assert list(new) == OLD_PARAMETERS + ["kp_cols32"]
    assert new["kp_cols32"].default is None
    for name in OLD_PARAMETERS[1:]:
        assert new[name].default == par[name].default or (new[name].default is None and par[name].default is None), name
    assert par["pd_stride"].default == 100 and par["nchunks"].default == 0 and par["eps"].default == 1e-6


def test_library_exports_it_and_refuses_null_arguments():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert hasattr(L, NAME) and re.search(r"\bT " + NAME + r"\b", out)
    io3 = _lib.StreamIO3()
    io3.struct_size = C.sizeof(_lib.StreamIO3)
    io3.io2.struct_size = C.sizeof(_lib.StreamIO2)
    assert L.kpilqr_iterate_streamed3(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed3(None, C.byref(io3), 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed2(None, None, 100, 3) == _lib.ERR_ARG             # the older entry points as before
    assert L.kpilqr_iterate_streamed(None, None, 100, 3) == _lib.ERR_ARG


def test_ctypes_struct_has_the_layout_of_the_c_compiler(tmp_path):
    c = tmp_path / "layout.c"
    prints = "".join(f'    printf("{f} %zu\\n", offsetof(kpilqr_stream_io3, {f}));\n' for f in FIELDS)
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "kpilqr.h"\nint main(void)\n{\n'
                 '    printf("sizeof %zu\\n", sizeof(kpilqr_stream_io3));\n    printf("sizeof_io2 %zu\\n", sizeof(kpilqr_stream_io2));\n'
                 '    printf("sizeof_io %zu\\n", sizeof(kpilqr_stream_io));\n'
                 + prints + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert [f for f, _ in _lib.StreamIO3._fields_] == FIELDS
    assert got["sizeof"] == C.sizeof(_lib.StreamIO3) and got["sizeof_io2"] == C.sizeof(_lib.StreamIO2)
    assert got["sizeof_io"] == C.sizeof(_lib.StreamIO)
    for f in FIELDS:
        assert got[f] == getattr(_lib.StreamIO3, f).offset, (f, got[f])


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("struct_size must be sizeof(kpilqr_stream_io3) as the caller compiled it",
                 "io2.struct_size sizeof(kpilqr_stream_io2)",
                 "with kp_columns32 = NULL the call IS kpilqr_iterate_streamed2 (one implementation, the same copies and launches in the same order)",
                 "one payload per iteration, at most one of the four may be given",
                 "kp_columns32 must be pinned (kpilqr_host_alloc)",
                 "Encoding and decoding are, word for word, those of kpilqr_upload_kp_columns_f32",
                 "kind-2 slots of DoFs >= num_ctrl are present and ignored",
                 "the state an iteration with io.kp_columns fed the decoded doubles leaves",
                 "nothing downstream knows the difference",
                 "all before anything is enqueued or the context is changed",
                 "The refusals of kpilqr_iterate_streamed2 keep their codes",
                 "a chunk without entries copies and launches nothing",
                 "as KPILQR_PIPE_COPY bit 0 says for every other upload",
                 "Consecutive calls with unchanged key-points overlap without a wait",
                 "share the buffer and order themselves behind a streamed iteration in flight",
                 "Out of scope: uploads or sweeps of a subset inside the chunks; KPILQR_FLAG_UNION_KEYPOINTS inside the chunks",
                 "the host classes (they do not use the streamed route)",
                 "any change to kpilqr_stream_io or kpilqr_stream_io2",
                 "detect the call by its symbol",
                 "Out of scope: the chunk pipeline (kpilqr_stream_io and kpilqr_stream_io2 are fixed structs"):   # the explicit call keeps its words
        assert word in doc, word


def test_no_new_environment_name():
    csrc = os.path.join(ROOT, "trajoptkp_amd", "csrc")
    assert "getenv" not in open(os.path.join(csrc, "columns_f32.hip")).read()
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")))
    read = set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src))
    assert not [n for n in read if "F32" in n or "COL" in n or "GAIN" in n or "STREAM" in n], read
