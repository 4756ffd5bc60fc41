"""CPU tests of the lambda retry schedule's boundary (kpilqr_set_lambda_retry / kpilqr_download_lambda_retry) and of the INPUTS of
tests/test_gpu_lambda_retry.py: the reference loop of tests/_lambda_retry.py has to show, for every problem the GPU tests run, a
trajectory that settles at once, one that needs three sweeps or more, and -- in a one-tile and in a tiled problem -- one that gives
up; otherwise the GPU tests would compare retries that never happen.  Then header, binding and built library agree on the two calls,
which refuse what they must before any device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import trajoptkp_amd
from trajoptkp_amd import _lib

import _lambda_retry as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kpilqr.h")).read()
FLAT = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S))       # declarations without their comments, on one line
SIGNATURES = {
    "kpilqr_set_lambda_retry": "kpilqr_ctx *ctx, const kpilqr_lambda_retry *sched",
    "kpilqr_download_lambda_retry": "kpilqr_ctx *ctx, double *lambda_used , int *attempts",
}


# ---- the inputs of the GPU tests: asserted before anything else -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lr.PROBLEMS))
def test_problem_has_the_attempt_counts_the_gpu_tests_rely_on(name):
    r = lr.reference(name)
    att = list(map(int, r["attempts"]))
    assert 1 in att, att
    assert max(att) >= 3, att
    assert np.any(r["settled"] & (r["attempts"] >= 3)), "nobody SETTLES after three sweeps or more"
    # the loop's own bookkeeping: lambda_used is the last lambda visited, every step is one multiply by the factor
    for b, seen in enumerate(r["visited"]):
        assert len(seen) == att[b] and seen[0] == lr.LAM0[b] and seen[-1] == r["lambda_used"][b]
        assert all(seen[i + 1] == seen[i] * lr.FACTOR for i in range(len(seen) - 1))
        assert r["lambda_used"][b] <= lr.MAX_LAMBDA
        if r["gave_up"][b]:
            assert r["status"][b] != 0 and r["lambda_used"][b] * lr.FACTOR > lr.MAX_LAMBDA
    assert bool(np.any(r["gave_up"])) == (name in lr.GIVE_UP), (name, r["gave_up"])


@pytest.mark.parametrize("name", sorted(lr.PROBLEMS))
def test_settled_sweeps_are_well_conditioned(name):
    """What the GPU tests hold to 1e-9 of the oracle must not amplify rounding by more than MAX_SENSITIVITY (tests/_lambda_retry.py)."""
    for sched in ({}, lr.OTHER_SCHEDULE):
        r = lr.reference(name, **sched)
        for b in np.nonzero(r["settled"])[0]:
            S = lr.sensitivity(name, int(b), float(r["lambda_used"][b]))
            assert S <= lr.MAX_SENSITIVITY, (name, sched, b, r["lambda_used"][b], S)


def test_a_one_tile_and_a_tiled_problem_give_up_and_every_case_names_a_problem():
    tiles = {name: (2 * trajoptkp_amd.synth.TASKS[lr.PROBLEMS[name][0]]["dof"] + 2 + 15) // 16 for name in lr.GIVE_UP}
    assert min(tiles.values()) == 1 and max(tiles.values()) >= 2, tiles
    for name in lr.GIVE_UP:
        r = lr.reference(name)
        assert np.any(r["gave_up"]) and np.any(r["settled"]), (name, r["status"])      # a MIXED batch: the gate has both kinds to keep apart
    assert {c[0] for c in lr.CASES.values()} == set(lr.PROBLEMS)


def test_caps_and_other_schedules_of_the_gpu_tests():
    full = lr.reference("panda")
    need3 = [b for b in range(4) if full["attempts"][b] == 3]
    assert need3, full["attempts"]
    capped = lr.reference("panda", max_attempts=2)
    for b in need3:                                 # out of attempts: failed, and one more multiply would still be allowed
        assert capped["attempts"][b] == 2 and capped["status"][b] != 0 and not capped["gave_up"][b]
        assert capped["lambda_used"][b] == lr.LAM0[b] * lr.FACTOR
    single = lr.reference("panda", max_attempts=1)
    assert list(single["attempts"]) == [1] * 4 and np.any(single["status"] != 0)
    for name in ("panda", "pushing"):
        other = lr.reference(name, **lr.OTHER_SCHEDULE)
        assert len(set(map(int, other["attempts"]))) >= 3 and np.any(other["settled"]), other["attempts"]
        for b, seen in enumerate(other["visited"]):
            assert all(seen[i + 1] == seen[i] * 4.0 for i in range(len(seen) - 1)) and seen[-1] <= 50.0


# ---- header, binding, library ----------------------------------------------------------------------------------------------------------
def test_header_declares_both_calls_and_the_struct():
    for name, args in SIGNATURES.items():
        m = re.search(r"\bint " + name + r"\(([^)]*)\)", FLAT)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args, (name, m.group(1))
    m = re.search(r"typedef struct \{([^}]*)\} kpilqr_lambda_retry;", FLAT)
    assert m and [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == ["struct_size", "factor", "max_lambda", "max_attempts"]
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by symbol: no version bump


def test_binding_mirrors_the_struct_and_lists_both_symbols():
    assert set(SIGNATURES) <= set(_lib.SYMBOLS) and set(SIGNATURES) <= _lib.OPTIONAL_SYMBOLS
    assert [(n, t) for n, t in _lib.LambdaRetry._fields_] == [("struct_size", C.c_size_t), ("factor", C.c_double), ("max_lambda", C.c_double),
                                                              ("max_attempts", C.c_int)]
    assert C.sizeof(_lib.LambdaRetry) == 32
    par = inspect.signature(trajoptkp_amd.Engine.set_lambda_retry).parameters
    assert [(k, v.default) for k, v in par.items()][1:] == [("factor", 10.0), ("max_lambda", 10.0), ("max_attempts", 6)]
    assert list(inspect.signature(trajoptkp_amd.Engine.lambda_retry).parameters) == ["self"]
    # existing signatures stay as they are
    assert list(inspect.signature(trajoptkp_amd.Engine.backward).parameters) == ["self", "lam", "pd_stride", "fetch"]
    assert list(inspect.signature(trajoptkp_amd.Engine.iterate).parameters) == ["self", "lam", "pd_stride", "alphas"]
    # kpilqr_stream_io / _io2 did not grow: the schedule is set on the context
    assert C.sizeof(_lib.StreamIO2) == C.sizeof(_lib.StreamIO) + 32 and "retry" not in " ".join(n for n, _ in _lib.StreamIO._fields_)


def test_library_exports_them_and_refuses_a_null_context():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in SIGNATURES:
        assert hasattr(L, name) and re.search(r"\bT " + name + r"\b", out), name
    s = _lib.LambdaRetry(C.sizeof(_lib.LambdaRetry), 10.0, 10.0, 6)
    assert L.kpilqr_set_lambda_retry(None, C.byref(s)) == _lib.ERR_ARG
    assert L.kpilqr_set_lambda_retry(None, None) == _lib.ERR_ARG
    assert L.kpilqr_download_lambda_retry(None, None, None) == _lib.ERR_ARG


def test_host_library_exports_the_new_runner_and_keeps_the_old():
    host_lib = os.path.join(os.path.dirname(_lib.LIB_PATH), "libkpilqr_host.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", host_lib], text=True)
    for name in ("kpilqr_host_run_acrobot_batch5", "kpilqr_host_run_acrobot_batch6"):
        assert re.search(r"\bT " + name + r"\b", out), name


def test_header_documents_the_contract():
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("lambda' = lambda * factor (ONE IEEE multiply)", "lambda' > max_lambda: give up", "fewer than max_attempts sweeps",
                 "NULL turns it off, the default", "the RESIDENT lambda is the lambda of its last sweep",
                 "A settled trajectory is never swept again within the call", "lambda exit", "out of attempts",
                 "kpilqr_resize keeps the schedule", "kpilqr_backward_stats ignores it", "either may be NULL",
                 "behind a streamed iteration in flight", "valid after kpilqr_sync",
                 "KPILQR_ERR_STATE while no schedule is set or before any backward sweep ran under it",
                 "max_attempts outside 1 .. 64", "detect the calls by their symbols"):
        assert word in doc, word


def _sweep_instantiations(direction, suffix):
    """The k_<direction>_* kernels in the device code of libkpilqr.so, split by their LAST template argument -- GATED of every backward
    kernel, LISTED of every forward one -- into two sets of (name, all other arguments, EXCL among them).
    generic.hip's kernels are no templates and keep the name suffix: k_backward_generic_retry is k_backward_generic<true> here."""
    out = subprocess.run(["strings", "-n", "12", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"_ZN6kpilqr\d+k_%s_\w+" % direction, out))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(syms)), capture_output=True, text=True, check=True).stdout.split("\n")
    kernels = {re.sub(r"^void ", "", n.split("(")[0]) for n in names if "k_%s_" % direction in n and "_stats" not in n}
    off, on = set(), set()
    for k in kernels:
        base, args = k.split("<", 1) if "<" in k else (k, ">")
        args = [a.strip() for a in args.rstrip(">").split(",")] if args != ">" else []
        if not args:
            assert "_generic" in base, k
            base, args = re.sub(suffix + "$", "", base), ["true" if base.endswith(suffix) else "false"]
        assert args[-1] in ("true", "false"), k
        (on if args[-1] == "true" else off).add((base, tuple(args[:-1])))
    return kernels, off, on


def test_built_library_holds_a_gated_twin_of_every_backward_kernel():
    """The device code of libkpilqr.so has, for every backward kernel instantiation that a backward pass launches, its lambda retry
    twin (the GATED = true instantiation of the same kernel, every other argument equal): as many twins as kernels, family by family."""
    kernels, plain, twins = _sweep_instantiations("backward", "_retry")
    assert len(kernels) > 100, len(kernels)
    assert plain == twins, (sorted(plain - twins)[:5], sorted(twins - plain)[:5])


def test_built_library_holds_a_listed_twin_of_every_forward_kernel():
    """... and for every forward kernel instantiation its LISTED = true partner (kpilqr_forward_linear_partial), and the other way round."""
    kernels, whole, listed = _sweep_instantiations("forward", "_listed")
    assert len(kernels) > 100, len(kernels)
    assert whole == listed, (sorted(whole - listed)[:5], sorted(listed - whole)[:5])
