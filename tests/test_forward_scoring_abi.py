"""CPU tests of the boundary of kpilqr_last_launch(ctx, 3), the scoring of the last forward launch ("pair2" | "step" | ""): the symbol
is in the built library with its signature, the header and the binding name the new selector, the version is unchanged, and a call
without a context answers "" without touching a device (tests/test_gpu_forward_paired_scoring.py runs the feature)."""
import os
import re
import subprocess

import trajoptkp_amd
from trajoptkp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "kpilqr.h")).read()


def test_library_exports_last_launch_and_answers_empty_without_a_context():
    L = trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert hasattr(L, "kpilqr_last_launch") and re.search(r"\bT kpilqr_last_launch\b", out)
    for which in (0, 1, 2, 3, 4, -1):
        assert L.kpilqr_last_launch(None, which) == b"", which


def test_header_documents_the_selector():
    assert re.search(r"const char \*kpilqr_last_launch\(kpilqr_ctx \*ctx, int which\);", HEADER)
    assert re.search(r"#define KPILQR_VERSION 410\b", HEADER)      # detected by the answer: no version bump
    doc = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", HEADER))      # comment blocks as running text
    for word in ("which = 3: how the last forward launch scored its steps", '"pair2"', '"step"', "n_alpha <= 8",
                 '"" before any forward launch', 'returns "" for which = 3 at all times; KPILQR_VERSION is unchanged'):
        assert word in doc, word


def test_binding_maps_forward_scoring_to_the_selector():
    calls = []

    class FakeLib:
        @staticmethod
        def kpilqr_last_launch(handle, which):
            calls.append(which)
            return b"pair2"

    e = object.__new__(trajoptkp_amd.Engine)
    e._L, e._h = FakeLib, None
    assert trajoptkp_amd.Engine.last_launch(e, "forward_scoring") == "pair2" and calls == [3]
    assert trajoptkp_amd.Engine.last_launch(e, "forward") == "pair2" and calls == [3, 1]
