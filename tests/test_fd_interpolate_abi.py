"""CPU tests of the kpilqr_fd_interpolate boundary: the header declares and documents it, the built library exports it without a
version bump, and the new kernels pass the ISA lint (hipcc cross-compiles without a GPU)."""
import os
import re
import subprocess
import sys

import trajoptkp_amd
from trajoptkp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kpilqr.h")).read()


def test_header_declares_the_entry_point():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bint\s+kpilqr_fd_interpolate\s*\(\s*kpilqr_ctx\s*\*\s*ctx\s*\)\s*;", code)


def test_header_documents_the_switch_and_the_stage_report():
    assert "KPILQR_FD_INTERP" in HEADER.split("#ifdef __cplusplus")[0]            # in the switch table at the top
    assert re.search(r"which = 2", HEADER)
    for name in ("fd_kp_interpolate", "kp_columns_interpolate", "fd_difference+interpolate", "in_sweep"):
        assert f'"{name}"' in HEADER, name
    assert "detect the entry point by its symbol" in HEADER.split("kpilqr_fd_interpolate(kpilqr_ctx")[0][-2500:]


def test_library_exports_the_symbol_and_keeps_its_version():
    L = trajoptkp_amd.load()
    assert hasattr(L, "kpilqr_fd_interpolate")
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT kpilqr_fd_interpolate\b", out)
    assert L.kpilqr_version() == 410
    assert int(re.search(r"#define KPILQR_VERSION (\d+)", HEADER).group(1)) == 410
    assert L.kpilqr_fd_interpolate(None) == _lib.ERR_ARG                            # a NULL context touches no device
    assert L.kpilqr_last_launch(None, 2) == b""


def test_the_binding_treats_the_entry_point_as_optional():
    assert "kpilqr_fd_interpolate" in _lib.SYMBOLS and "kpilqr_fd_interpolate" in _lib.OPTIONAL_SYMBOLS


def test_linearise_kernels_pass_the_isa_lint():
    """No scratch and no waterfall loop in k_fd_kp_interpolate<false> / <true> (tools/isa_lint.py)."""
    src = os.path.join(ROOT, "trajoptkp_amd", "csrc", "linearise.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), "--strict", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "linearise.hip: 2 kernels" in r.stdout, r.stdout
    for waterfall, scratch in re.findall(r"waterfall loops (\d+), .*?scratch (\d+) B", r.stdout):
        assert int(waterfall) == 0 and int(scratch) == 0, r.stdout
    # the lint itself reads ScratchSize from the assembly: make sure both kernels were seen there with 0 bytes
    asm = subprocess.check_output(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                                   "-o", "-", src], text=True, stderr=subprocess.DEVNULL)
    sizes = re.findall(r"^; ScratchSize: (\d+)", asm, flags=re.M)
    assert len(sizes) == 2 and all(int(x) == 0 for x in sizes), sizes
    assert "k_fd_kp_interpolateILb0" in asm and "k_fd_kp_interpolateILb1" in asm


def test_makefile_builds_linearise_without_contraction():
    mk = open(os.path.join(ROOT, "trajoptkp_amd", "csrc", "Makefile")).read()
    rule = re.search(r"\$\(OBJ\)/linearise\.o:.*\n(?:\t.*\n)+", mk).group(0)
    assert "$(STRICT)" in rule and "-ffp-contract=off" in mk and "$(OBJ)/linearise.o" in mk.split("OBJS :=")[1].split("\n")[0]
