"""CPU tests of the boundary of kpilqr_iterate_streamed5 (the chunk pipeline linearising and sweeping a listed subset of the batch): the
struct and the call exist in the header, the binding and the built library, the ctypes structure has the C compiler's layout, a NULL
context or struct is refused before anything touches a device, and the header says what a caller has to know
(tests/test_gpu_streamed_sweeps.py runs the feature)."""
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
NAME = "kpilqr_iterate_streamed5"
FIELDS = ["struct_size", "io4", "sweep_count", "sweep_traj"]
OLD_PARAMETERS = ["self", "fd", "fd_kp", "kp_cols", "eps", "r", "r_x", "r_u", "u_nom", "lam", "K", "k", "cost_pred", "delta_J", "status",
                  "pd_stride", "nchunks", "K32", "gain_traj"]
ENVIRONMENT = {"KPILQR_FUSED_WAVES", "KPILQR_FUSED_FWD_WAVES", "KPILQR_ROLE_SHIFT", "KPILQR_TILED_NT_MIN", "KPILQR_TILED_A6",
               "KPILQR_TILED_UW", "KPILQR_TILED_FSC", "KPILQR_PIPE_COPY", "KPILQR_FUSED_RAW", "KPILQR_FUSED_UNI", "KPILQR_FD_INTERP"}


def members(struct):
    m = re.search(r"typedef struct \{([^{}]*)\} " + struct + ";", FLAT)
    assert m, struct
    return [re.sub(r"\s+", " ", x).strip() for x in m.group(1).split(";") if x.strip()]


def test_header_declares_the_struct_and_the_call():
    assert members("kpilqr_stream_io5") == ["size_t struct_size", "kpilqr_stream_io4 io4", "int sweep_count", "const int *sweep_traj"]
    m = re.search(r"\bint " + NAME + r"\(([^)]*)\)", FLAT)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "kpilqr_ctx *ctx, const kpilqr_stream_io5 *io5, int pd_check_stride, int nchunks"
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump
    assert trajoptkp_amd.load().kpilqr_version() == 410
    # the older structs keep their members
    assert members("kpilqr_stream_io4") == ["size_t struct_size", "kpilqr_stream_io3 io3", "int upload_count", "const int *upload_traj"]
    assert members("kpilqr_stream_io3") == ["size_t struct_size", "kpilqr_stream_io2 io2", "const float *kp_columns32"]
    assert members("kpilqr_stream_io2") == ["size_t struct_size", "kpilqr_stream_io io", "float *K32", "int gain_count", "const int *gain_traj"]


def test_binding_lists_the_symbol_and_keeps_the_old_signatures():
    assert NAME in _lib.SYMBOLS and NAME in _lib.OPTIONAL_SYMBOLS
    par = inspect.signature(trajoptkp_amd.Engine.iterate_streamed).parameters
    assert list(par) == OLD_PARAMETERS
    assert list(inspect.signature(trajoptkp_amd.Engine.iterate_streamed3).parameters) == OLD_PARAMETERS + ["kp_cols32"]
    four = inspect.signature(trajoptkp_amd.Engine.iterate_streamed4).parameters
    assert list(four) == OLD_PARAMETERS + ["kp_cols32", "upload_traj"]
    new = inspect.signature(trajoptkp_amd.Engine.iterate_streamed5).parameters
    assert list(new) == OLD_PARAMETERS + ["kp_cols32", "upload_traj", "sweep_traj"]
    assert new["sweep_traj"].default is None and new["upload_traj"].default is None and new["kp_cols32"].default is None
    for name in list(four)[1:]:
        assert new[name].default == four[name].default or (new[name].default is None and four[name].default is None), name
    assert par["pd_stride"].default == 100 and par["nchunks"].default == 0 and par["eps"].default == 1e-6


def sized_io5():
    io5 = _lib.StreamIO5()
    io5.struct_size = C.sizeof(_lib.StreamIO5)
    io5.io4.struct_size = C.sizeof(_lib.StreamIO4)
    io5.io4.io3.struct_size = C.sizeof(_lib.StreamIO3)
    io5.io4.io3.io2.struct_size = C.sizeof(_lib.StreamIO2)
    return io5


def test_library_exports_it_and_refuses_null_arguments():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert hasattr(L, NAME) and re.search(r"\bT " + NAME + r"\b", out)
    io5 = sized_io5()
    assert L.kpilqr_iterate_streamed5(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed5(None, C.byref(io5), 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed4(None, None, 100, 3) == _lib.ERR_ARG             # the older entry points as before
    assert L.kpilqr_iterate_streamed4(None, C.byref(io5.io4), 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed3(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed2(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed(None, None, 100, 3) == _lib.ERR_ARG


def test_ctypes_struct_has_the_layout_of_the_c_compiler(tmp_path):
    c = tmp_path / "layout.c"
    prints = "".join(f'    printf("{f} %zu\\n", offsetof(kpilqr_stream_io5, {f}));\n' for f in FIELDS)
    sizes = "".join(f'    printf("sizeof_{s} %zu\\n", sizeof(kpilqr_stream_{s}));\n' for s in ("io5", "io4", "io3", "io2", "io"))
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "kpilqr.h"\nint main(void)\n{\n' + sizes + prints + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert [f for f, _ in _lib.StreamIO5._fields_] == FIELDS
    for s, t in (("io5", _lib.StreamIO5), ("io4", _lib.StreamIO4), ("io3", _lib.StreamIO3), ("io2", _lib.StreamIO2), ("io", _lib.StreamIO)):
        assert got["sizeof_" + s] == C.sizeof(t), s
    for f in FIELDS:
        assert got[f] == getattr(_lib.StreamIO5, f).offset, (f, got[f])


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("struct_size must be sizeof(kpilqr_stream_io5) as the caller compiled it",
                 "with sweep_traj = NULL the call IS kpilqr_iterate_streamed4 (one implementation, the same copies and launches in the same order",
                 "sweep_count is then ignored unless it is > 0, which is refused",
                 "sweep_traj [sweep_count] is strictly increasing and within [0, batch)",
                 "read during the call only and may be pageable",
                 "handled as kpilqr_iterate_partial handles them",
                 "the launches of kpilqr_fd_interpolate_partial and kpilqr_cost_derivs_partial",
                 "No byte of an unlisted trajectory's K, k, status, delta_J, cost_pred, lambda, attempts or step records is written",
                 "io.lambda [sweep_count] in list order, placed by one k_rows_in launch per chunk",
                 "io.cost_pred [sweep_count][n_alpha], io.delta_J and io.status [sweep_count]",
                 "nothing beyond sweep_count rows is written",
                 "gain_traj is independent of sweep_traj",
                 "which must be a subset of sweep_traj (a re-linearised trajectory is an active one)",
                 "an upload_traj entry missing from sweep_traj (the error names it)",
                 "The pending-range rule of kpilqr_iterate_streamed4 after kpilqr_update_keypoints is unchanged",
                 "sweep_count = 0 with a list: nothing is swept and nothing is uploaded; the gains of gain_traj still come down",
                 "then kpilqr_iterate_partial for sweep_traj with the compact lambdas",
                 'reports the forms with ":subset" last, on every kind of context',
                 "a listed sweep reads the column store and never differences inside the sweep",
                 "the chunk runs the differencing and slope launches over its own entry range on its own stream",
                 "KPILQR_FLAG_UNION_KEYPOINTS is ignored",
                 "follows the length of the chunk's slice of the list on the chunk's share of the SIMDs",
                 "the schedule arms listed trajectories only",
                 "follows the chunk's slice of the compact lambdas (io.lambda = NULL: max_attempts)",
                 "all before anything is enqueued or the context is changed (a context in the constant-Jacobian mode stays in it)",
                 "sweep_count < 0, sweep_count > 0 with a NULL list",
                 "KPILQR_ERR_STATE before any key-points exist",
                 "Every refusal of the older calls keeps its code",
                 "A chunk without listed trajectories launches nothing but its share of the gain download",
                 "one gathering launch per chunk and array (k_rows_out, rows_in.hip) straight into the caller's pinned buffer",
                 "two consecutive calls with different sweep lists overlap without a wait",
                 "a context that never passes one allocates and launches nothing new",
                 "Out of scope: differencing inside a listed sweep, or proportional to the list; job-list payloads with any list",
                 "(since: kpilqr_iterate_streamed5, below, linearises and sweeps a listed subset inside the chunks.)",
                 "detect the call by its symbol"):
        assert word in doc, word


def test_no_new_environment_name():
    csrc = os.path.join(ROOT, "trajoptkp_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")))
    assert set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src)) == ENVIRONMENT
