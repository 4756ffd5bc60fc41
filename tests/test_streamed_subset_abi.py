"""CPU tests of the boundary of kpilqr_iterate_streamed4 (the chunk pipeline uploading the inputs of a listed subset of the batch): the
struct and the call exist in the header, the binding and the built library, the ctypes structure has the C compiler's layout, a NULL
context or struct is refused before anything touches a device, and the header says what a caller has to know
(tests/test_gpu_streamed_subset.py runs the feature)."""
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
NAME = "kpilqr_iterate_streamed4"
FIELDS = ["struct_size", "io3", "upload_count", "upload_traj"]
OLD_PARAMETERS = ["self", "fd", "fd_kp", "kp_cols", "eps", "r", "r_x", "r_u", "u_nom", "lam", "K", "k", "cost_pred", "delta_J", "status",
                  "pd_stride", "nchunks", "K32", "gain_traj"]


def test_header_declares_the_struct_and_the_call():
    m = re.search(r"typedef struct \{([^{}]*)\} kpilqr_stream_io4;", FLAT)
    assert m, "kpilqr_stream_io4"
    members = [re.sub(r"\s+", " ", x).strip() for x in m.group(1).split(";") if x.strip()]
    assert members == ["size_t struct_size", "kpilqr_stream_io3 io3", "int upload_count", "const int *upload_traj"], members
    m = re.search(r"\bint " + NAME + r"\(([^)]*)\)", FLAT)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "kpilqr_ctx *ctx, const kpilqr_stream_io4 *io4, int pd_check_stride, int nchunks"
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump
    assert trajoptkp_amd.load().kpilqr_version() == 410
    # the older structs keep their members
    m3 = re.search(r"typedef struct \{([^{}]*)\} kpilqr_stream_io3;", FLAT)
    assert [re.sub(r"\s+", " ", x).strip() for x in m3.group(1).split(";") if x.strip()] == \
        ["size_t struct_size", "kpilqr_stream_io2 io2", "const float *kp_columns32"]


def test_binding_lists_the_symbol_and_keeps_the_old_signatures():
    assert NAME in _lib.SYMBOLS and NAME in _lib.OPTIONAL_SYMBOLS
    par = inspect.signature(trajoptkp_amd.Engine.iterate_streamed).parameters
    assert list(par) == OLD_PARAMETERS
    three = inspect.signature(trajoptkp_amd.Engine.iterate_streamed3).parameters
    assert list(three) == OLD_PARAMETERS + ["kp_cols32"]
    new = inspect.signature(trajoptkp_amd.Engine.iterate_streamed4).parameters
    assert list(new) == OLD_PARAMETERS + ["kp_cols32", "upload_traj"]
    assert new["upload_traj"].default is None and new["kp_cols32"].default is None
    for name in list(three)[1:]:
        assert new[name].default == three[name].default or (new[name].default is None and three[name].default is None), name
    assert par["pd_stride"].default == 100 and par["nchunks"].default == 0 and par["eps"].default == 1e-6


def test_library_exports_it_and_refuses_null_arguments():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert hasattr(L, NAME) and re.search(r"\bT " + NAME + r"\b", out)
    io4 = _lib.StreamIO4()
    io4.struct_size = C.sizeof(_lib.StreamIO4)
    io4.io3.struct_size = C.sizeof(_lib.StreamIO3)
    io4.io3.io2.struct_size = C.sizeof(_lib.StreamIO2)
    assert L.kpilqr_iterate_streamed4(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed4(None, C.byref(io4), 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed3(None, None, 100, 3) == _lib.ERR_ARG             # the older entry points as before
    assert L.kpilqr_iterate_streamed2(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed(None, None, 100, 3) == _lib.ERR_ARG


def test_ctypes_struct_has_the_layout_of_the_c_compiler(tmp_path):
    c = tmp_path / "layout.c"
    prints = "".join(f'    printf("{f} %zu\\n", offsetof(kpilqr_stream_io4, {f}));\n' for f in FIELDS)
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "kpilqr.h"\nint main(void)\n{\n'
                 '    printf("sizeof %zu\\n", sizeof(kpilqr_stream_io4));\n    printf("sizeof_io3 %zu\\n", sizeof(kpilqr_stream_io3));\n'
                 '    printf("sizeof_io2 %zu\\n", sizeof(kpilqr_stream_io2));\n    printf("sizeof_io %zu\\n", sizeof(kpilqr_stream_io));\n'
                 + prints + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert [f for f, _ in _lib.StreamIO4._fields_] == FIELDS
    assert got["sizeof"] == C.sizeof(_lib.StreamIO4) and got["sizeof_io3"] == C.sizeof(_lib.StreamIO3)
    assert got["sizeof_io2"] == C.sizeof(_lib.StreamIO2) and got["sizeof_io"] == C.sizeof(_lib.StreamIO)
    for f in FIELDS:
        assert got[f] == getattr(_lib.StreamIO4, f).offset, (f, got[f])


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("struct_size must be sizeof(kpilqr_stream_io4) as the caller compiled it",
                 "io3.struct_size sizeof(kpilqr_stream_io3) and io3.io2.struct_size sizeof(kpilqr_stream_io2)",
                 "with upload_traj = NULL the call IS kpilqr_iterate_streamed3 (one implementation, the same copies and launches in the same order",
                 "upload_traj [upload_count] is strictly increasing and within [0, batch)",
                 "it is read during the call only and may be pageable; it is independent of gain_traj",
                 "the listed trajectories' rows back to back in list order; a NULL pointer keeps what is resident",
                 "at most one of io.fd_kp_slab, io.kp_columns, io3.kp_columns32 may be given",
                 "io.entries is the sum of their entry counts under the CURRENT lists",
                 "io.lambda stays [batch]",
                 "upload_count = 0 with a list: no input but lambda is copied",
                 "whole-batch arrays that hold the resident bytes with the listed rows / entries replaced",
                 "K, k, cost_pred, delta_J and status bit for bit",
                 "still run over every trajectory of every chunk",
                 "A streamed4 call whose payload list contains every pending trajectory completes them",
                 "A list that misses a pending trajectory is KPILQR_ERR_STATE naming it",
                 "all before anything is enqueued or the context is changed (a context in the constant-Jacobian mode stays in it)",
                 "io.fd_slab together with a list",
                 "io.entries that is not the listed sum",
                 "no complete resident payload of the same kind for the trajectories not listed (kp_columns32 counts as the column kind)",
                 "the refusals of kpilqr_upload_residuals_partial, in its words",
                 "Every refusal of the older calls keeps its code",
                 "ONE launch of k_rows_in (rows_in.hip)",
                 "as KPILQR_PIPE_COPY bit 0 says for every other upload",
                 "A chunk without listed trajectories copies and launches nothing for the inputs beyond lambda",
                 "Two consecutive calls with DIFFERENT lists overlap like calls with equal lists",
                 "addressed by the chunk (its first trajectory), not by the list",
                 "staging as large as the whole-batch form of each input kind that was ever given with a list",
                 "KPILQR_ERR_ALLOC when it cannot be had",
                 "first orders itself behind the iteration in flight",
                 "A context that never passes a list allocates and launches nothing new",
                 "Out of scope: sweeps or linearisation of a subset; job-list payloads (io.fd_slab) with a list; KPILQR_FLAG_UNION_KEYPOINTS inside the chunks",
                 "the host classes and the batch shim (they do not use the streamed route)",
                 "detect the call by its symbol"):
        assert word in doc, word


def test_no_new_environment_name():
    csrc = os.path.join(ROOT, "trajoptkp_amd", "csrc")
    assert "getenv" not in open(os.path.join(csrc, "rows_in.hip")).read()
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")))
    read = set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src))
    assert read == {"KPILQR_FUSED_WAVES", "KPILQR_FUSED_FWD_WAVES", "KPILQR_ROLE_SHIFT", "KPILQR_TILED_NT_MIN", "KPILQR_TILED_A6",
                    "KPILQR_TILED_UW", "KPILQR_TILED_FSC", "KPILQR_PIPE_COPY", "KPILQR_FUSED_RAW", "KPILQR_FUSED_UNI", "KPILQR_FD_INTERP"} \
        or not [n for n in read if "ROWS" in n or "SUBSET" in n or "UPLOAD" in n or "STREAM" in n or "LIST" in n], read
