"""The short-horizon table of tests/_horizons.py against the sources and the oracle (no GPU): the step groups are the ones the
.hip files define, every loop is met below, at and above one full group and at every residue by the forms that run it, every
case dispatches to the variant its form names, the oracle settles every trajectory, and the per-DoF cases have per-DoF lists."""
import numpy as np
import pytest

import _horizons as HZ
import _shapes as S
from _shape_run import _problem
from oracle import pipeline

N_SIMD = 1024          # an MI355X (256 CUs x 4); the GPU tests read it from the device
CASES = HZ.cases()


def missing_horizons(group, horizons, t_min, block=False):
    """What a loop of `group` steps still lacks when the forms that run it run `horizons` (t_min: the shortest horizon those
    forms can run at all)."""
    hs = set(horizons)
    lack = []
    if t_min < group and not any(T < group for T in hs):
        lack.append("below")
    lack += [f"T={T}" for T in (group, group + 1) if T >= t_min and T not in hs and not (block and T == group + 1)]
    if block:
        lack += [f"T={group - 1}"] if group - 1 not in hs else []
    else:
        # (every residue on a horizon of at least one full group: below it the body never runs and the tail alone decides)
        lack += [f"residue {r}" for r in range(group) if not any(T % group == r for T in hs if T >= group)]
    return lack


def test_groups_are_the_sources():
    assert HZ.parsed_groups() == HZ.GROUPS


def test_a_changed_set_count_is_noticed(tmp_path):
    import os, shutil
    for name in {v[0] for v in HZ._SOURCES.values()}:
        shutil.copy(os.path.join(HZ.CSRC, name), tmp_path / name)
    p = tmp_path / "fused_mfma.hip"
    p.write_text(p.read_text().replace("#define KP_FWD_SETS 4 ", "#define KP_FWD_SETS 5 "))
    assert HZ.parsed_groups(str(tmp_path)) != HZ.GROUPS


def test_case_ids_are_unique():
    ids = [HZ.case_id(c) for c in CASES] + [HZ.failure_id(c) for c in HZ.failure_cases()]
    assert len(set(ids)) == len(ids)


def _horizons_by_loop():
    by = {loop: [] for loop in HZ.GROUPS}
    for c in CASES:
        for loop in HZ.loops_of(c, N_SIMD):
            by[loop].append(c)
    return by


@pytest.mark.parametrize("loop", sorted(HZ.GROUPS))
def test_every_loop_meets_every_horizon(loop):
    cs = _horizons_by_loop()[loop]
    assert cs, loop
    group = HZ.GROUPS[loop]
    if loop in HZ.BLOCK_LOOPS:                          # the block edges, over the forms together (two forms carry T = 15, 16)
        assert S._case(1, 1, 1, 0)["T"] == group + 1    # one above a block: the default horizon of tests/_shapes.py
        assert missing_horizons(group, [c["T"] for c in cs], 2, True) == []
        return
    # a pipelined loop: the horizon list of EVERY form that runs it, on its own
    for form in sorted({c["form"] for c in cs}):
        # per-DoF lists exist from T = 4 on (bisect_keypoints: at T <= 3 every list is (0, T-1)); kpilqr_create takes T >= 2
        t_min = 2 if HZ.FORMS[form][6] else 4
        assert all(loop in HZ.loops_of(c, N_SIMD) for c in CASES if c["form"] == form), (loop, form)
        assert missing_horizons(group, HZ.FORMS[form][7], t_min) == [], (loop, form)


def test_a_dropped_residue_is_noticed():
    assert missing_horizons(4, (2, 3, 4, 5, 7, 8, 9), 2) == ["residue 2"]
    assert missing_horizons(6, range(4, 13), 4) == []
    assert missing_horizons(6, range(6, 14), 4) == ["below"]
    assert missing_horizons(4, (4, 5, 6, 7), 4) == []
    assert missing_horizons(2, (2, 4), 2) == ["T=3", "residue 1"]
    assert missing_horizons(16, (2, 15, 16), 2, block=True) == []
    assert missing_horizons(2, (4, 5), 4) == []             # (per-DoF forms start at T = 4: a two-step group has no T = 2, 3 there)
    assert missing_horizons(2, (4, 6), 4) == ["residue 1"]


def test_the_table_names_the_forms_of_the_issue():
    forms = {c["form"] for c in CASES}
    assert {f"fused_w1_d{n // 2}" for n, _ in S.T1_SHAPES} | {f"t1_d{n // 2}" for n, _ in S.T1_SHAPES} <= forms
    assert len(CASES) >= 250
    for c in CASES:
        if c["form"] in HZ.LAYOUT_FORMS and c["min_N"] != 4:
            assert c["T"] in HZ.H_LAYOUT and c["min_N"] in (1, 2)
        assert c["batch"] == 2 and c["n_alpha"] == 6
        assert c["kp_ordered"] == (bool(c["flags"] & S.FLAG_FUSED) and c["T"] % 2 == 1)


@pytest.mark.parametrize("c", CASES + HZ.failure_cases(), ids=[HZ.case_id(c) for c in CASES] + [HZ.failure_id(c) for c in HZ.failure_cases()])
def test_case_dispatches_to_its_variant(c):
    d = S.dispatch(c["dof"], c["m"], c["nr"], c["T"], c["n_alpha"], c["batch"], N_SIMD, c["flags"], c["env"], c["rx_const"], True,
                   c["uniform"])
    assert d is not None
    want_fwd = {"wide_d12": "mfma_f64_tiled"}.get(c["form"], c["variant"])          # (m = 9: the tiled forward takes it, _shapes.py:52)
    assert d["variants"] == (c["variant"], want_fwd), (d["variants"], c)
    compiled = set(S.COMPILED)
    for key in (d["bwd"], d["fwd"]) + tuple(d["extra"]):
        assert key in compiled, (key, c)
    env = c["env"]
    if c["variant"] == "mfma_f64_t1_fused":            # the wave forms the form's environment asks for
        want_b = ":w1:" if env["KPILQR_FUSED_WAVES"] == "1" else ":pairh:"
        fw = env["KPILQR_FUSED_FWD_WAVES"]
        want_f = {"1": ":w1:", "3": ":triple:", "4": ":pair:" if c["uniform"] else ":triple:"}[fw]
        assert want_b in d["launch"][0] and want_f in d["launch"][1], (d["launch"], c)


def test_the_six_set_loop_is_reached():
    """KPILQR_FUSED_FWD_WAVES = 4 on a per-DoF set runs the triple at this batch (plan_forward_fused); the general one-wave
    form with r_u = 0 -- six sets -- needs "1"."""
    by = _horizons_by_loop()
    assert {c["form"] for c in by["fused_fwd_gen_ru0"]} == {"fused_ragged_rxc_w1_d7", "fused_ragged_rxc_w1_d2"}
    assert all("fused_fsc" in HZ.loops_of(c, N_SIMD) for c in CASES if c["form"].startswith("fused_ragged_rxc_d"))


@pytest.mark.parametrize("c", CASES, ids=[HZ.case_id(c) for c in CASES])
def test_oracle_settles_and_lists_differ(c):
    p = _problem(c, min_N=c["min_N"])
    for b in range(p["batch"]):
        o = pipeline.run_trajectory(p, b, n_alpha=c["n_alpha"], stages=("fd", "interp", "cost", "bwd"))
        assert o["status"] == 0, (HZ.case_id(c), b)
        if not c["uniform"]:
            offs, cols = p["kp_rows"][b]
            lists = [tuple(t for t in range(c["T"]) if d in cols[offs[t]:offs[t + 1]]) for d in range(c["dof"])]
            assert len(set(lists)) > 1, (HZ.case_id(c), b, lists)
            assert all(l[0] == 0 and l[-1] == c["T"] - 1 for l in lists)


@pytest.mark.parametrize("c", HZ.failure_cases(), ids=[HZ.failure_id(c) for c in HZ.failure_cases()])
def test_failure_is_where_it_was_put(c):
    p = HZ.failing_problem(_problem(c), c["t_star"])
    st = [pipeline.run_trajectory(p, b, pd_stride=1, stages=("fd", "interp", "cost", "bwd"))["status"] for b in range(2)]
    assert st == [0, c["t_star"] + 1]
    assert np.any(p["r_u"][0])                          # r_u is streamed
