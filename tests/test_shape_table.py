"""The dispatch table of tests/_shapes.py against itself (no GPU): every instantiation the library compiles has at least one
case in tests/test_gpu_shapes.py, every case reaches compiled instantiations only (or is a stated refusal), and the chooser's
smallest / largest shapes are what the launchers' rules say."""
import pytest

import _shapes as S

N_SIMD = 1024          # an MI355X (256 CUs x 4); the GPU tests read it from the device


def _all_cases():
    return S.cases(N_SIMD) + S.batch_cases(N_SIMD)


def test_every_compiled_key_has_a_case():
    covered = set()
    for c in _all_cases():
        covered.update(S.case_keys(c, N_SIMD))
    missing = [k for k in S.COMPILED if k not in covered]
    assert not missing, missing


def test_every_case_maps_to_a_compiled_key_or_a_stated_refusal():
    compiled = set(S.COMPILED)
    assert len(compiled) == len(S.COMPILED)
    for c in _all_cases():
        d = S.dispatch(c["dof"], c["m"], c["nr"], c["T"], c["n_alpha"], c["batch"], N_SIMD, c["flags"], c["env"], c["rx_const"],
                       True, c["uniform"])
        if c["why"] == "refused":
            assert d is None, c
            continue
        assert d is not None, c
        for key in (d["bwd"], d["fwd"]) + tuple(d["extra"]):
            assert key in compiled, (key, c)


def test_generic_lds_bound_for_seven_controls():
    # select_variants (kpilqr_api.cpp) with generic.hip:93: 19 970 doubles at dof 46 fit in 160 KB, 20 774 at dof 47 do not
    assert S.GENERIC_MAX_DOF_M7 == 46
    assert S.generic_lds_bytes(92, 7) <= 160 * 1024 < S.generic_lds_bytes(94, 7)
    assert S.select_variants(46, 7, 4, 5, 6, 2, 0) == ("generic_lds", "generic_lds")
    assert S.select_variants(47, 7, 4, 5, 6, 2, 0) is None
    assert S.select_variants(32, 7, 4, 5, 6, 2, 0) == ("generic_lds", "generic_lds")     # five state tiles: no MFMA family


@pytest.mark.parametrize("key,dofs", [(("tiled_bwd", 7, 2, 3, "uw"), (12, 13)),        # n = 24, 26: NT = 2, NCL = 3
                                      (("tiled_bwd", 7, 2, 1, "uw"), (1, 9)),          # (a state smaller than one tile runs one chunk)
                                      (("tiled_bwd", 7, 3, 4, "uw"), (22, 23)),
                                      (("tiled_bwd", 7, 4, 1, "col"), (24, 25)),
                                      (("tiled_bwd", 7, 4, 4, "col"), (30, 31)),
                                      (("wide_bwd", 2, 1), (1, 15))])
def test_chooser_extremes(key, dofs):
    got = S.chooser(N_SIMD)[key]
    assert (got[0]["dof"], got[-1]["dof"]) == dofs, [(c["dof"], c["m"]) for c in got]


def test_fused_shapes_and_residual_chunks():
    assert [S.rv2_ncr(nr) for nr in (1, 2, 8, 9, 10, 16)] == [1, 2, 2, 3, 4, 4]
    assert S.select_variants(7, 7, 16, 17, 16, 2, S.FLAG_FUSED) == ("mfma_f64_t1_fused",) * 2
    assert S.select_variants(7, 7, 17, 17, 6, 2, S.FLAG_FUSED) == ("mfma_f64_t1", "mfma_f64_t1")       # nr = 17: not fused
    assert S.select_variants(7, 7, 4, 17, 17, 2, S.FLAG_FUSED) == ("mfma_f64_t1", "generic_lds")       # n_alpha = 17
    assert S.select_variants(12, 7, 17, 17, 6, 2, S.FLAG_FUSED, {"KPILQR_TILED_A6": "1"}) == ("mfma_f64_tiled",) * 2
    assert S.select_variants(2, 3, 2, 17, 6, 2, S.FLAG_FUSED) == ("mfma_f64_tiled", "mfma_f64_t1")     # m > dof: never fused
