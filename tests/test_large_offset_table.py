"""The large-offset table of tests/_large_offsets.py against itself, the dispatch table and the sources (no GPU): every family has a
case past 2^31 elements and one (or a named case of the same template) with K past 2^32 bytes, every case fits the memory cap, no
truncation of a checked offset lands on data of the same seed and step, every case dispatches to its family, and the in-trajectory
horizon limits are the ones the sources have."""
import functools
import shutil

import numpy as np
import pytest

import _large_offsets as LO
import _shapes as S
from oracle import pipeline

N_SIMD = 1024          # an MI355X (256 CUs x 4); the GPU tests read it from the device


@functools.lru_cache(maxsize=None)
def _problem(name):
    return LO.problem(LO.BY_NAME[name])


def test_the_table_is_printed():
    print("\n" + LO.table())
    assert len({c["name"] for c in LO.CASES}) == len(LO.CASES) == len(LO.EXPECT)


# ---- thresholds ------------------------------------------------------------------------------------------------------------------
def _families(cases):
    return {f: [c for c in cases if f in c["families"]] for f in LO.FAMILIES}


def missing_thresholds(cases):
    """[(family, what)] a case table still lacks"""
    by_name = {c["name"]: c for c in cases}
    lack = []
    for fam, cs in _families(cases).items():
        if not any(LO.largest_input(c)[1] > 2 ** 31 for c in cs):
            lack.append((fam, "no case whose largest input buffer is past 2^31 elements"))
        k_cases = [c for c in cs if LO.buffers(c)["K"]["bytes"] > 2 ** 32]
        for c in cs:                                                    # a case that names a carrier: it exists, has K past 2^32 bytes ...
            if c["k_carrier"] is not None:
                k = by_name.get(c["k_carrier"])
                if k is None or LO.buffers(k)["K"]["bytes"] <= 2 ** 32 or fam not in k["families"]:
                    lack.append((fam, f"{c['name']}: its K carrier {c['k_carrier']} does not carry"))
        if not k_cases:
            lack.append((fam, "no case with K past 2^32 bytes"))
    return lack


def test_every_family_crosses_every_threshold():
    assert missing_thresholds(LO.CASES) == []
    assert all(c["families"] and set(c["families"]) <= set(LO.FAMILIES) for c in LO.CASES)


def test_a_lost_threshold_is_noticed():
    smaller = [dict(c, reps=c["reps"] - 1, batch=(c["reps"] - 1) * LO.UNIQ) if c["name"] == "tiled_col_2" else c for c in LO.CASES]
    assert ("tiled_col_a6", "tiled_col_4: its K carrier tiled_col_2 does not carry") in missing_thresholds(smaller)
    without = [c for c in LO.CASES if c["name"] != "generic"]
    assert ("generic", "no case with K past 2^32 bytes") in missing_thresholds(without)
    short = [dict(c, reps=2613, batch=2613 * LO.UNIQ) if c["families"] == ("fused_waves",) else c for c in LO.CASES]
    assert ("fused_waves", "no case whose largest input buffer is past 2^31 elements") in missing_thresholds(short)


@pytest.mark.parametrize("c", LO.CASES, ids=LO.case_id)
def test_a_carrier_runs_the_same_kernel_template(c):
    if c["k_carrier"] is None:
        return
    k = LO.BY_NAME[c["k_carrier"]]
    key = lambda x: S.dispatch(x["dof"], x["m"], x["nr"], x["T"], x["n_alpha"], x["batch"], N_SIMD, x["flags"], x["env"], x["rx_const"], True, x["uniform"])["bwd"]
    a, b = key(c), key(k)
    assert a[0] == b[0] == "tiled_bwd" and a[4] == b[4], (a, b)          # the form (uw | col | a6) of k_backward_tiled*; NT, NCL, M differ
    reps_k = 2 ** 32 // (8 * 2 * c["dof"] * c["m"] * c["T"] * LO.UNIQ) + 1                     # the replicas that would put this shape's K past 2^32 bytes ...
    assert LO.total_bytes(dict(c, reps=reps_k, batch=reps_k * LO.UNIQ)) > LO.CAP               # ... do not fit


# ---- memory cap --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LO.CASES, ids=LO.case_id)
def test_case_fits_the_memory_cap(c):
    assert LO.total_bytes(c) <= LO.CAP, (c["name"], LO.total_bytes(c))
    assert c["batch"] == c["reps"] * LO.UNIQ and LO.UNIQ == 7
    assert 100 <= c["T"] < 1000                                          # the batch carries the offset
    assert all(len(l) >= 3 for u in range(LO.UNIQ) for l in LO.kp_lists(c, u))
    # the host side stays small: the payload, and the UNIQ trajectories' arrays
    assert LO.buffers(c)["payload"]["bytes"] < 2 ** 30


# ---- no aliasing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LO.CASES, ids=LO.case_id)
def test_no_truncated_offset_lands_on_the_same_data(c):
    held = LO.held_buffers(c)
    assert "K" in held or c["k_carrier"] is not None
    name, el = LO.largest_input(c)
    if el > 2 ** 31:
        assert name in held, (name, sorted(held))
    for buf, b in held.items():
        wrapped, same = LO.aliased(c, buf, b)
        assert wrapped > 0 and same == 0, (c["name"], buf, wrapped, same)
    p = _problem(c["name"])
    for buf in ("r", "r_x", "r_u", "u_nom"):
        if buf in held:
            assert LO.inputs_differ(c, p, buf, held[buf]) == 0, (c["name"], buf)


def test_an_aliasing_batch_is_noticed():
    """A horizon and a replica count that are powers of two: trajectory b and b - 2^k carry the same seed at the same step."""
    c = dict(LO.BY_NAME["t1_plain"], T=512, reps=2048, batch=2048 * LO.UNIQ)
    b = dict(inner=512, unit=2 ** 12, elem=8, bytes=c["batch"] * 512 * 2 ** 12 * 8)           # 2^24 bytes per trajectory
    wrapped, same = LO.aliased(c, "records", b)
    assert wrapped > 0 and same == 0                                     # 7 is odd: a shift of 2^k trajectories changes the seed
    # ... and with an even number of seeds it does not: the same code on a replica map of 8
    import unittest.mock as mock
    with mock.patch.object(LO, "UNIQ", 8):
        c8 = dict(c, batch=2048 * 8)
        wrapped, same = LO.aliased(c8, "records", dict(b, bytes=c8["batch"] * 512 * 2 ** 12 * 8))
    assert wrapped > 0 and same == wrapped


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LO.CASES, ids=LO.case_id)
def test_case_dispatches_to_its_family(c):
    d = S.dispatch(c["dof"], c["m"], c["nr"], c["T"], c["n_alpha"], c["batch"], N_SIMD, c["flags"], c["env"], c["rx_const"], True, c["uniform"])
    bv, fv, lb, lf = LO.EXPECT[c["name"]]
    assert d["variants"] == (bv, fv), (c["name"], d)
    assert {d["bwd"], d["fwd"]} | set(d["extra"]) <= set(S.COMPILED)
    want = {"t1_plain": ("t1_bwd", "plain"), "tiled_uw_2_fwd": ("tiled_bwd", "uw"), "tiled_uw_2_fsc": ("tiled_bwd", "uw"), "tiled_uw_3": ("tiled_bwd", "uw"),
            "tiled_col_4": ("tiled_bwd", "col"), "tiled_col_2": ("tiled_bwd", "col"), "tiled_a6_4": ("tiled_bwd", "a6"), "tiled_a6_2": ("tiled_bwd", "a6"),
            "wide_m9": ("wide_bwd", 1), "wide_m17": ("wide_bwd", 2), "generic": ("generic_bwd", "generic_bwd")}.get(c["name"])
    if want:
        assert d["bwd"][0] == want[0] and d["bwd"][-1] == want[1], (c["name"], d["bwd"])
    nt = {"tiled_uw_2_fwd": 2, "tiled_uw_2_fsc": 2, "tiled_uw_3": 3, "tiled_col_4": 4, "tiled_a6_4": 4, "tiled_col_2": 2, "tiled_a6_2": 2}.get(c["name"])
    if nt:
        assert d["bwd"][2] == nt
    assert (d["fwd"][0] == "tiled_fwd_sc") == (c["name"] == "tiled_uw_2_fsc")
    if c["name"] == "tiled_uw_2_fwd":
        assert d["fwd"][0] == "tiled_fwd"
    waves = {"fused_w1_raw_uni": ("w1", "w1"), "fused_w1_ragged": ("w1", "w1"), "fused_w1_rxc": ("w1", "w1"), "fused_pairh_pair": ("pairh", "pair"),
             "fused_w1_triple": ("w1", "triple")}.get(c["name"])
    assert (waves is not None) == LO.is_fused(c)
    if waves:
        assert (d["bwd"][3], d["fwd"][3]) == waves and d["bwd"][4] in ("plain", "-"), (c["name"], d)
        assert ("fused_rv2" in [k[0] for k in d["extra"]]) == (c["name"] == "fused_w1_rxc")


# ---- the oracle settles, the trajectories are distinct ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1_plain", "fused_w1_ragged", "fused_w1_rxc", "tiled_uw_2_fwd", "wide_m17"])
def test_oracle_settles_and_seeds_differ(name):
    c, p = LO.BY_NAME[name], _problem(name)
    refs = [pipeline.run_trajectory(p, u, n_alpha=c["n_alpha"], want_U=True) for u in range(LO.UNIQ)]
    assert all(o["status"] == 0 for o in refs)
    assert len(np.unique([o["cost_pred"][0] for o in refs])) == LO.UNIQ and len(np.unique([o["delta_J"] for o in refs])) == LO.UNIQ
    if not c["uniform"]:
        assert all(len({tuple(l) for l in LO.kp_lists(c, u)}) > 1 for u in range(LO.UNIQ))
    offs, times = LO.tiled_csr(p, 3)
    o1, t1 = LO.dof_csr(dict(p, kp_rows=p["kp_rows"] * 3))
    assert np.array_equal(offs, o1) and np.array_equal(times, t1)


# ---- horizon limits ---------------------------------------------------------------------------------------------------------------
def test_cited_constants_are_the_sources():
    assert LO.stale_citations() == []
    assert S.FSC_REC_BYTES_MAX == 0x7fffff00 and S.BIGOFF == 0x40000000


def test_a_changed_constant_is_noticed(tmp_path):
    import os
    for name in {cite[0] for spec in LO.HORIZON_LIMITS.values() for cite in spec["cites"]}:
        shutil.copy(os.path.join(LO.CSRC, name), tmp_path / name)
    p = tmp_path / "tiled_mfma.hip"
    p.write_text(p.read_text().replace("#define KP_FSC_REC_BYTES_MAX 0x7fffff00u", "#define KP_FSC_REC_BYTES_MAX 0xffffff00u"))
    assert [s[0] for s in LO.stale_citations(str(tmp_path))] == ["tiled_fsc_records"]
    p = tmp_path / "fused_mfma.hip"
    p.write_text(p.read_text().replace("#define BIGOFF 0x40000000", "#define BIGOFF 0x20000000"))
    assert {s[0] for s in LO.stale_citations(str(tmp_path))} == {"tiled_fsc_records", "fused_payload"}


def test_horizon_limits():
    print()
    for form, spec in LO.HORIZON_LIMITS.items():
        print(f"{form}: {spec['what']}\n    guard: {spec['guard']}\n    cited: " + ", ".join(f"{n}:{l}" for n, l, _ in spec["cites"]))
    # the fused sweeps: the guard of fused_supported is what _shapes.fused_supported restates, and every per-trajectory descriptor of
    # the forward sweeps stays below 2^31 bytes at the longest horizon the guard lets through, at the largest nr
    for n, m in S.T1_SHAPES:
        dof = n // 2
        T_max = LO.HORIZON_LIMITS["fused_payload"]["max_T"](dof, m, 16)
        assert S.fused_supported(n, m, 16, dof, T_max, 6) and not S.fused_supported(n, m, 16, dof, T_max + 1, 6)
        assert LO.HORIZON_LIMITS["fused_forward_descriptors"]["max_T"](dof, m, 16) >= T_max, (n, m)
        print(f"    fused ({n}, {m}): T <= {T_max}")
    # the state / cost waves: every two-tile shape the form takes has a record larger than K's step, so the record bound comes first;
    # under it the form is selected, beyond it not -- whatever KPILQR_TILED_FSC says
    for dof in range(1, 16):
        for m in range(1, 9):
            n = 2 * dof
            if S.tiled_nt(n) != 2:
                continue
            T_in = LO.HORIZON_LIMITS["tiled_fsc_records"]["max_T"](dof, m, 4)
            assert S.rec_stride(n, m) > m * n and LO.HORIZON_LIMITS["tiled_fsc_gains"]["max_T"](dof, m, 4) > T_in
            assert T_in * S.rec_stride(n, m) * 8 <= S.FSC_REC_BYTES_MAX < (T_in + 1) * S.rec_stride(n, m) * 8
            for env in ({"KPILQR_TILED_FSC": "1"}, {}):
                fwd = lambda T: S.dispatch(dof, m, 4, T, 6, 1, N_SIMD, S.FLAG_TILED, env)
                assert fwd(T_in)["fwd"][0] == "tiled_fwd_sc" and ":state_cost_waves" in fwd(T_in)["launch"][1]
                assert fwd(T_in + 1)["fwd"][0] == "tiled_fwd" and ":state_cost_waves" not in fwd(T_in + 1)["launch"][1]
    assert (LO.FSC_T_INSIDE, LO.FSC_T_BEYOND) == (125203, 125204) and S.rec_stride(30, 8) == 2144
    # reachable under the cap: one trajectory of the widest two-tile shape at the first horizon beyond the limit is 2 GB of records
    assert LO.FSC_T_BEYOND * S.rec_stride(30, 8) * 8 < 3 << 30
