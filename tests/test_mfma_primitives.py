"""CPU test of the primitive layer of the MFMA sweep units (riccati_mfma.hip, forward_mfma.hip, tiled_mfma.hip, tiled_wide.hip,
fused_mfma.hip): the matrix instruction and the buffer descriptor are spelled in mfma_common.h alone, and none of the private copies
the units carried (renamed aliases of the same few lines) is defined again.  Reads source text only; compiles nothing."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trajoptkp_amd", "csrc")
SOURCES = {os.path.basename(p): open(p).read() for ext in ("hip", "h", "cpp") for p in sorted(glob.glob(os.path.join(CSRC, "*." + ext)))}

MFMA = "__builtin_amdgcn_mfma_f64_16x16x4f64"
RSRC = "__builtin_amdgcn_make_buffer_rsrc"
# Raw descriptor calls that stay outside the header, by file: (count, reason).  Each was tried through kp_rsrc and changed the device
# text of the kernels named (profiles/mfma_primitives_isa.txt); identical text outranks the wrapper.
RSRC_EXCEPTIONS = {
    "riccati_mfma.hip": (2, "rK, rk of store_gains: through kp_rsrc the four k_backward_mfma<4, 1, ...> kernels change"),
    "tiled_mfma.hip": (6, "the a6 source descriptors of load_cost / cost_rsrc in k_backward_tiled_col: through kp_rsrc the sixteen "
                          "<7 | 8, 4, true, NCL > 0, ...> kernels change"),
}
DELETED = ("WMFMA", "OOBT", "OOBF", "OOBW", "tbld", "fbld", "wbld", "frsrc", "wlds", "wsts", "WPn", "fset_reg", "WideSrc")


def test_sources_found():
    assert "mfma_common.h" in SOURCES and len(SOURCES) >= 20
    assert MFMA in SOURCES["mfma_common.h"] and RSRC in SOURCES["mfma_common.h"]


def test_matrix_instruction_spelled_in_the_header_alone():
    assert [name for name, text in SOURCES.items() if MFMA in text] == ["mfma_common.h"]


def test_descriptor_spelled_in_the_header_alone():
    found = {name: text.count(RSRC) for name, text in SOURCES.items() if RSRC in text and name != "mfma_common.h"}
    assert found == {name: count for name, (count, _) in RSRC_EXCEPTIONS.items()}, found
    assert SOURCES["mfma_common.h"].count(RSRC) == 1                     # kp_rsrc


def test_deleted_private_names_are_not_defined_again():
    again = []
    for name, text in SOURCES.items():
        for word in DELETED:
            w = r"\b" + word + r"\b"
            if (re.search(r"^\s*#\s*define\s+" + w, text, re.M) or re.search(r"\bstruct\s+" + w, text)
                    or re.search(r"\btypedef\b[^;]*" + w + r"[^;]*;", text)
                    or re.search(r"^[^\n;/]*__device__[^\n;{(]*" + w + r"\s*\(", text, re.M)):
                again.append((name, word))
    assert not again, again
