"""CPU tests of the boundary of kpilqr_iterate_streamed2 (the chunk pipeline with K as FP32 and the gains of a list of trajectories):
the struct and the call exist in the header, the binding and the built library, the ctypes structure has the C compiler's layout,
a NULL context or struct is refused before anything touches a device, and the header says what a caller has to know
(tests/test_gpu_streamed_gains.py runs the feature)."""
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
NAME = "kpilqr_iterate_streamed2"
FIELDS = ["struct_size", "io", "K32", "gain_count", "gain_traj"]


def test_header_declares_the_struct_and_the_call():
    m = re.search(r"typedef struct \{([^{}]*)\} kpilqr_stream_io2;", FLAT)
    assert m, "kpilqr_stream_io2"
    members = [re.sub(r"\s+", " ", x).strip() for x in m.group(1).split(";") if x.strip()]
    assert members == ["size_t struct_size", "kpilqr_stream_io io", "float *K32", "int gain_count", "const int *gain_traj"], members
    m = re.search(r"\bint " + NAME + r"\(([^)]*)\)", FLAT)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "kpilqr_ctx *ctx, const kpilqr_stream_io2 *io2, int pd_check_stride, int nchunks"
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump
    assert trajoptkp_amd.load().kpilqr_version() == 410


def test_binding_lists_the_symbol_and_keeps_the_old_parameters():
    assert NAME in _lib.SYMBOLS and NAME in _lib.OPTIONAL_SYMBOLS
    par = inspect.signature(trajoptkp_amd.Engine.iterate_streamed).parameters
    assert list(par) == ["self", "fd", "fd_kp", "kp_cols", "eps", "r", "r_x", "r_u", "u_nom", "lam", "K", "k", "cost_pred", "delta_J", "status",
                         "pd_stride", "nchunks", "K32", "gain_traj"]
    assert par["K32"].default is None and par["gain_traj"].default is None
    assert par["pd_stride"].default == 100 and par["nchunks"].default == 0 and par["eps"].default == 1e-6


def test_library_exports_it_and_refuses_null_arguments():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert hasattr(L, NAME) and re.search(r"\bT " + NAME + r"\b", out)
    io2 = _lib.StreamIO2()
    io2.struct_size = C.sizeof(_lib.StreamIO2)
    assert L.kpilqr_iterate_streamed2(None, None, 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed2(None, C.byref(io2), 100, 3) == _lib.ERR_ARG
    assert L.kpilqr_iterate_streamed(None, None, 100, 3) == _lib.ERR_ARG              # the old entry point as before


def test_ctypes_struct_has_the_layout_of_the_c_compiler(tmp_path):
    c = tmp_path / "layout.c"
    prints = "".join(f'    printf("{f} %zu\\n", offsetof(kpilqr_stream_io2, {f}));\n' for f in FIELDS)
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "kpilqr.h"\nint main(void)\n{\n'
                 '    printf("sizeof %zu\\n", sizeof(kpilqr_stream_io2));\n    printf("sizeof_io %zu\\n", sizeof(kpilqr_stream_io));\n'
                 + prints + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert [f for f, _ in _lib.StreamIO2._fields_] == FIELDS
    assert got["sizeof"] == C.sizeof(_lib.StreamIO2) and got["sizeof_io"] == C.sizeof(_lib.StreamIO)
    for f in FIELDS:
        assert got[f] == getattr(_lib.StreamIO2, f).offset, (f, got[f])


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("struct_size must be sizeof(kpilqr_stream_io2) as the caller compiled it",
                 "the outputs are COMPACT: K (or K32) [gain_count][T][n][m] and k [gain_count][T][m]",
                 "nothing beyond gain_count rows is written",
                 "strictly increasing and within [0, batch) -- the contract of kpilqr_download_gains_partial",
                 "gain_count = 0 with a list: no gains come down",
                 "gain_traj is read during the call only and may be pageable",
                 "io.K and K32 are exclusive",
                 "K32 must be pinned (kpilqr_host_alloc) and 8-byte aligned",
                 "the IEEE round-to-nearest-even cast of the resident FP64 K, bit for bit",
                 "FP32 subnormals are produced, not flushed", "become +-inf", "NaN stays NaN",
                 "k stays FP64", "The resident FP64 K is only read",
                 "The sweeps run over the whole batch regardless of the list",
                 "cost_pred, delta_J and status stay whole-batch outputs",
                 "all before anything is enqueued or the context is changed",
                 "take this route whatever KPILQR_PIPE_COPY says",
                 "Bit 1 does not reach the K32 and gain_traj downloads of kpilqr_iterate_streamed2",
                 "no staging buffer, no second DMA",
                 "detect the call by its symbol",
                 "Out of scope: kpilqr_iterate_streamed"):                   # the FP32 paragraph keeps its words: true of that entry point
        assert word in doc, word


def test_gains_hip_reads_no_environment():
    csrc = os.path.join(ROOT, "trajoptkp_amd", "csrc")
    assert "getenv" not in open(os.path.join(csrc, "gains.hip")).read()
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")))
    read = set(re.findall(r'(?:env_int|getenv)\("(KPILQR_[A-Z0-9_]+)"', src))
    assert not [n for n in read if "F32" in n or "GAIN" in n or "STREAM" in n], read
