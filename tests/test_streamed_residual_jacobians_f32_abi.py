"""CPU tests of the boundary of kpilqr_iterate_streamed6 (the chunk pipeline taking the per-step residual Jacobians as FP32): the struct
and the call exist in the header, the binding and the built library, the ctypes structure has the C compiler's layout down to
kpilqr_stream_io, a NULL context or struct is refused before anything touches a device, and the header says what a caller has to know
(tests/test_gpu_streamed_residual_jacobians_f32.py runs the feature).  A library without the symbol fails these tests."""
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
DOC = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))                      # comment blocks as running text
NAME = "kpilqr_iterate_streamed6"
FIELDS = ["struct_size", "io5", "r_x32", "r_u32"]
OLD_PARAMETERS = ["self", "fd", "fd_kp", "kp_cols", "eps", "r", "r_x", "r_u", "u_nom", "lam", "K", "k", "cost_pred", "delta_J", "status",
                  "pd_stride", "nchunks", "K32", "gain_traj"]
ENVIRONMENT = {"KPILQR_FUSED_WAVES", "KPILQR_FUSED_FWD_WAVES", "KPILQR_ROLE_SHIFT", "KPILQR_TILED_NT_MIN", "KPILQR_TILED_A6",
               "KPILQR_TILED_UW", "KPILQR_TILED_FSC", "KPILQR_PIPE_COPY", "KPILQR_FUSED_RAW", "KPILQR_FUSED_UNI", "KPILQR_FD_INTERP"}
SINCE = "(since: kpilqr_iterate_streamed6, below, takes the per-step residual Jacobians as FP32 inside the chunks.)"


def members(struct):
    m = re.search(r"typedef struct \{([^{}]*)\} " + struct + ";", FLAT)
    assert m, struct
    return [re.sub(r"\s+", " ", x).strip() for x in m.group(1).split(";") if x.strip()]


def test_header_declares_the_struct_and_the_call():
    assert members("kpilqr_stream_io6") == ["size_t struct_size", "kpilqr_stream_io5 io5", "const float *r_x32", "const float *r_u32"]
    m = re.search(r"\bint " + NAME + r"\(([^)]*)\)", FLAT)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "kpilqr_ctx *ctx, const kpilqr_stream_io6 *io6, int pd_check_stride, int nchunks"
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump
    assert trajoptkp_amd.load().kpilqr_version() == 410
    # the older structs keep their members
    assert members("kpilqr_stream_io5") == ["size_t struct_size", "kpilqr_stream_io4 io4", "int sweep_count", "const int *sweep_traj"]
    assert members("kpilqr_stream_io4") == ["size_t struct_size", "kpilqr_stream_io3 io3", "int upload_count", "const int *upload_traj"]
    assert members("kpilqr_stream_io3") == ["size_t struct_size", "kpilqr_stream_io2 io2", "const float *kp_columns32"]
    assert members("kpilqr_stream_io2") == ["size_t struct_size", "kpilqr_stream_io io", "float *K32", "int gain_count", "const int *gain_traj"]


def test_binding_lists_the_symbol_and_keeps_the_old_signatures():
    assert NAME in _lib.SYMBOLS and NAME in _lib.OPTIONAL_SYMBOLS
    par = inspect.signature(trajoptkp_amd.Engine.iterate_streamed).parameters
    assert list(par) == OLD_PARAMETERS
    assert list(inspect.signature(trajoptkp_amd.Engine.iterate_streamed3).parameters) == OLD_PARAMETERS + ["kp_cols32"]
    assert list(inspect.signature(trajoptkp_amd.Engine.iterate_streamed4).parameters) == OLD_PARAMETERS + ["kp_cols32", "upload_traj"]
    five = inspect.signature(trajoptkp_amd.Engine.iterate_streamed5).parameters
    assert list(five) == OLD_PARAMETERS + ["kp_cols32", "upload_traj", "sweep_traj"]
    new = inspect.signature(trajoptkp_amd.Engine.iterate_streamed6).parameters
    assert list(new) == list(five) + ["r_x32", "r_u32"]
    assert new["r_x32"].default is None and new["r_u32"].default is None
    for name in list(five)[1:]:
        assert new[name].default == five[name].default or (new[name].default is None and five[name].default is None), name
    assert par["pd_stride"].default == 100 and par["nchunks"].default == 0 and par["eps"].default == 1e-6


def sized_io6():
    io6 = _lib.StreamIO6()
    io6.struct_size = C.sizeof(_lib.StreamIO6)
    io6.io5.struct_size = C.sizeof(_lib.StreamIO5)
    io6.io5.io4.struct_size = C.sizeof(_lib.StreamIO4)
    io6.io5.io4.io3.struct_size = C.sizeof(_lib.StreamIO3)
    io6.io5.io4.io3.io2.struct_size = C.sizeof(_lib.StreamIO2)
    return io6


def test_library_exports_it_and_refuses_null_arguments():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert hasattr(L, NAME) and re.search(r"\bT " + NAME + r"\b", out)
    io6 = sized_io6()
    assert L.kpilqr_iterate_streamed6(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed6(None, C.byref(io6), 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed5(None, None, 100, 3) == _lib.ERR_ARG             # the older entry points as before
    assert L.kpilqr_iterate_streamed5(None, C.byref(io6.io5), 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed4(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed3(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed2(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed(None, None, 100, 3) == _lib.ERR_ARG


def test_ctypes_struct_has_the_layout_of_the_c_compiler(tmp_path):
    c = tmp_path / "layout.c"
    chain = (("io6", _lib.StreamIO6, FIELDS), ("io5", _lib.StreamIO5, ["struct_size", "io4", "sweep_count", "sweep_traj"]),
             ("io4", _lib.StreamIO4, ["struct_size", "io3", "upload_count", "upload_traj"]),
             ("io3", _lib.StreamIO3, ["struct_size", "io2", "kp_columns32"]),
             ("io2", _lib.StreamIO2, ["struct_size", "io", "K32", "gain_count", "gain_traj"]))
    io_fields = {"fd_slab": "fd_slab", "r": "r", "r_x": "r_x", "r_u": "r_u", "lambda": "lam", "K": "K", "status": "status", "entries": "entries",
                 "kp_columns": "kp_columns"}
    prints = "".join(f'    printf("{s}.{f} %zu\\n", offsetof(kpilqr_stream_{s}, {f}));\n' for s, _, fields in chain for f in fields)
    prints += "".join(f'    printf("io.{f} %zu\\n", offsetof(kpilqr_stream_io, {f}));\n' for f in io_fields)
    sizes = "".join(f'    printf("sizeof_{s} %zu\\n", sizeof(kpilqr_stream_{s}));\n' for s in ("io6", "io5", "io4", "io3", "io2", "io"))
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "kpilqr.h"\nint main(void)\n{\n' + sizes + prints + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert [f for f, _ in _lib.StreamIO6._fields_] == FIELDS
    for s, t, fields in chain + (("io", _lib.StreamIO, []),):
        assert got["sizeof_" + s] == C.sizeof(t), s
        for f in fields:
            assert got[f"{s}.{f}"] == getattr(t, f).offset, (s, f, got[f"{s}.{f}"])
    for f, py in io_fields.items():
        assert got["io." + f] == getattr(_lib.StreamIO, py).offset, f
    # the innermost struct sits where the chain of offsets says
    inner = sum(getattr(t, f).offset for t, f in ((_lib.StreamIO6, "io5"), (_lib.StreamIO5, "io4"), (_lib.StreamIO4, "io3"), (_lib.StreamIO3, "io2"),
                                                 (_lib.StreamIO2, "io")))
    assert inner == sum(got[k] for k in ("io6.io5", "io5.io4", "io4.io3", "io3.io2", "io2.io"))


def test_header_documents_the_contract():
    for word in ("struct_size must be sizeof(kpilqr_stream_io6) as the caller compiled it",
                 "with r_x32 = NULL and r_u32 = NULL the call IS kpilqr_iterate_streamed5 (one implementation, the same copies and launches in the same order)",
                 "r_x32 [batch][T+1][nr][n] and r_u32 [batch][T+1][nr][m] in the layout of io.r_x / io.r_u",
                 "[upload_count][T+1][nr][n] and [upload_count][T+1][nr][m], compact in list order",
                 "Both must be pinned (kpilqr_host_alloc) and 8-byte aligned",
                 "Per array, one transport per call: io.r_x together with r_x32, or io.r_u together with r_u32, is KPILQR_ERR_ARG",
                 "FP64 r_x beside r_u32, and the reverse, is allowed",
                 "any payload kind including kp_columns32, K32, gain_traj, upload_traj, sweep_traj, the lambda retry",
                 "Encoding and decoding are, word for word, those of kpilqr_upload_residual_jacobians_f32",
                 "the caller makes a plain (float) cast, the library widens exactly, dst = (double)src",
                 "FP32 subnormals widen to their value, +-inf stays +-inf, -0 stays -0, NaN stays NaN",
                 "bit for bit, those of a kpilqr_iterate_streamed5 given FP64 io.r_x / io.r_u that hold the widened floats",
                 "a whole r_x32 ends the constant-Jacobian mode, r_u32 counts r_u as non-zero",
                 "recorded behind every check that can still reject the call",
                 "the three refusals of kpilqr_upload_residuals_partial apply, with its code (KPILQR_ERR_STATE) and in its words",
                 "inputs come with an upload_traj inside sweep_traj, r_x32 or r_u32 without one is KPILQR_ERR_ARG",
                 "all before anything is enqueued or the context is changed (a context in the constant-Jacobian mode stays in it)",
                 "ctx = NULL or io6 = NULL, a wrong outer or inner struct_size, r_x32 or r_u32 not pinned or not 8-byte aligned",
                 "Every refusal of the older calls keeps its code",
                 "ONE launch serves BOTH arrays (k_widen_jacobians, residuals_f32.hip",
                 "a scattered list costs no copy per run",
                 "an array that is not given costs no block",
                 "r_u in pairs where (T+1)*nr*m is even and in single elements (4-byte loads, 8-byte stores) where it is odd",
                 "nothing beyond 4-byte alignment is assumed of it",
                 "The source follows KPILQR_PIPE_COPY bit 0, as every other upload does",
                 "laid out [r_x32 | r_u32] at whole-batch size",
                 "the launch reads the caller's pinned floats itself; no staging buffer is reserved or touched",
                 "A chunk without rows copies and launches nothing for the Jacobians",
                 "A region of the staging buffer is addressed by the chunk alone",
                 "share the buffer and order themselves behind a streamed iteration in flight",
                 "A context that never passes r_x32 / r_u32 allocates and launches nothing new",
                 "7.06 MB of residual Jacobians per trajectory become 3.53 MB",
                 "profiles/streamed_residual_jacobians_f32.txt",
                 "Out of scope: FP32 for r, u_nom or k, or inside any sweep; the host classes and the batch shim",
                 "KPILQR_VERSION is unchanged: detect the call by its symbol"):
        assert word in DOC, word
    # one appended line under the f32-Jacobian paragraph and under the streamed3 / streamed4 / streamed5 paragraphs
    assert DOC.count(SINCE) == 4
    for before in ("int kpilqr_upload_residual_jacobians_f32(", "} kpilqr_stream_io3;", "} kpilqr_stream_io4;", "} kpilqr_stream_io5;"):
        head = DOC[:DOC.index(before)]
        assert head.rstrip().rsplit("typedef struct", 1)[0].rstrip().endswith(SINCE + " */") or head.rstrip().endswith(SINCE + " */"), before
    # what the explicit calls' paragraph said about the gap stays, word for word
    assert "Out of scope: FP32 residual Jacobians inside the chunks of kpilqr_iterate_streamed* (a change of its own, as it was for the columns)" in DOC


def test_embed_paragraph_names_the_call():
    par = DOC[DOC.index("Out of scope on an embedded context"):]
    par = par[:par.index("*/")]
    assert re.search(r"\b" + NAME + r"\b", par)
    for older in ("kpilqr_iterate_streamed,", "kpilqr_iterate_streamed2", "kpilqr_iterate_streamed3", "kpilqr_iterate_streamed4", "kpilqr_iterate_streamed5"):
        assert older in par, older
    api = open(os.path.join(ROOT, "trajoptkp_amd", "csrc", "kpilqr_api.cpp")).read()
    assert f'KP_NOT_EMBEDDED(c, "{NAME}")' in api


def test_no_new_environment_name():
    csrc = os.path.join(ROOT, "trajoptkp_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")))
    assert set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src)) == ENVIRONMENT
