"""CPU tests of the boundary of key-point placement for a listed subset of the batch: the three entry points exist in the header, the
binding and the built library with the documented signatures, a NULL context is refused, and the header says what a caller has to
know (tests/test_gpu_keypoints_partial.py runs the feature)."""
import inspect
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
    "kpilqr_upload_states_partial": "kpilqr_ctx *ctx, int count, const int *traj, const double *X",
    "kpilqr_generate_keypoints_partial": "kpilqr_ctx *ctx, int count, const int *traj, const char *method, int min_N, int max_N, const double *thresholds, double dt",
    "kpilqr_get_keypoints_partial": "kpilqr_ctx *ctx, int count, const int *traj, int *kp_offsets , int *kp_times , int times_capacity",
}


def test_header_declares_the_three_entry_points():
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", FLAT)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args, (name, m.group(1))
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump


def test_binding_lists_them_as_optional_symbols():
    assert set(SIGNATURES) <= set(_lib.SYMBOLS) and set(SIGNATURES) <= _lib.OPTIONAL_SYMBOLS
    for name in ("upload_states_partial", "generate_keypoints_partial", "get_keypoints_partial"):
        assert callable(getattr(trajoptkp_amd.Engine, name)), name
    par = inspect.signature(trajoptkp_amd.Engine.generate_keypoints_partial).parameters
    assert list(par) == ["self", "traj", "method", "min_N", "max_N", "thresholds", "dt"]
    assert par["max_N"].default == 1 and par["thresholds"].default is None and par["dt"].default == 0.0
    assert list(inspect.signature(trajoptkp_amd.Engine.upload_states_partial).parameters) == ["self", "traj", "X"]
    assert list(inspect.signature(trajoptkp_amd.Engine.get_keypoints_partial).parameters) == ["self", "traj"]


def test_library_exports_them_and_refuses_a_null_context():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in SIGNATURES:
        assert hasattr(L, name) and re.search(r"\bT " + name + r"\b", out), name
    # a NULL context is refused before anything touches a device
    assert L.kpilqr_upload_states_partial(None, 0, None, None) == _lib.ERR_ARG
    assert L.kpilqr_generate_keypoints_partial(None, 0, None, b"set_interval", 2, 1, None, 0.0) == _lib.ERR_ARG
    assert L.kpilqr_get_keypoints_partial(None, 0, None, None, None, 0) == _lib.ERR_ARG


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("Key-point placement for a subset", "strictly increasing and within [0, batch)", "count = 0 is a no-op returning KPILQR_OK",
                 "a NULL context is KPILQR_ERR_ARG", "each call orders itself behind a streamed iteration in flight",
                 # the states of a subset
                 "X [count][T][n], the listed trajectories' states COMPACT in `traj` order",
                 "one hipMemcpyAsync per run of adjacent trajectories: no staging buffer, no kernel",
                 "one host byte per trajectory that says whether its states were ever given",
                 "a whole kpilqr_upload_states sets all of them, kpilqr_resize clears them",
                 # the placement
                 '"iterative_error" is refused with the same message',
                 "leaves the context exactly as kpilqr_update_keypoints(count, traj, lists) would",
                 "bit for bit what kpilqr_generate_keypoints with the same arguments and states places",
                 "the listed ranges PENDING until kpilqr_upload_fd_kp_partial / kpilqr_upload_kp_columns[_f32]_partial fills them",
                 "the union lists invalid, the host mirror of the offsets valid", "canonical, and uniform only for set_interval",
                 "before any key-points exist", "while ranges are pending after an earlier update",
                 "the message names the first such trajectory", "A rejected call leaves the context as it was",
                 # costs and waits
                 "a scalar load", "WAITS for ONE read-back of the count*dof counts", "no worst-case count*dof*T reservation of list times is made",
                 "from there the two calls are one function",
                 # the compact read-back
                 "kp_offsets [count*dof + 1] re-based to 0", "one copy per run of adjacent trajectories",
                 "Returns the number of entries of the listed trajectories", "Synchronous, like kpilqr_get_keypoints",
                 "kp_times = NULL queries the size and does not touch the device when the offsets mirror is valid",
                 "A times_capacity that is too small is KPILQR_ERR_ARG", "It works on any lists, not only device-placed ones",
                 "it is allowed while ranges are pending: it reads lists, not payload",
                 "Out of scope: the host shims"):
        assert word in doc, word
    # a "(since: ...)" note under each of the three older sentences that named the gap
    assert doc.count("(since: kpilqr_upload_states_partial and kpilqr_generate_keypoints_partial") == 2
    assert "(since: kpilqr_generate_keypoints_partial places key-points for a listed subset" in doc
    for old in ("and kpilqr_generate_keypoints places key-points for the whole batch only.",
                "kpilqr_generate_keypoints and kpilqr_upload_states for a subset; keeping",
                "kpilqr_generate_keypoints and kpilqr_upload_states for a subset; an environment switch."):
        assert old in doc, old                                      # the sentences themselves stay
