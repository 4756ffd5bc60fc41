"""The shortest horizons of every sweep family: the step groups of the software-pipelined time loops (read from the sources),
which loops a case of tests/_shapes.py runs, and the table of cases that meets every loop below, at and above one full group
and at every residue.  tests/test_horizon_table.py checks the table against the sources and the oracle (no GPU);
tests/test_gpu_horizons.py runs every case, and a PD failure pinned to a chosen step of a short horizon.

A sweep preloads NS register sets, runs a body of NS steps and then a tail; a request that would fall beyond the horizon is
clamped to a valid record (or made through an empty descriptor).  tests/_shapes.py runs T = 17 and T = 131 only: residue 1 of
every two-step group, 1 and 3 of the four-step groups, 5 of the six-step group, and no horizon below a group.

File:line citations are to trajoptkp_amd/csrc."""
import os
import re

import _shapes as S
from _shapes import FLAG_FUSED, FLAG_GENERIC, FLAG_TILED, T1_SHAPES, TILED_ENVS, _case

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trajoptkp_amd", "csrc")

# loop -> steps per group (register sets of the time loop, ring slots, steps per block)
GROUPS = {
    "ric_t1": 2,                # KP_RIC_SETS, riccati_mfma.hip:61: preload :133-136, request :186, pair loop and tail :302-311
    "fwd_t1": 2,                # Tiles S[2], forward_mfma.hip:92: preload :93-94, request :101, pair loop and odd step :133-134
    "fused_fwd_uni": 4,         # KP_FWD_SETS, fused_mfma.hip:50: NS :1620, preload :1654, request :1730, fwd_steps / fwd_tail :1881-1882
    "fused_fwd_gen": 4,         # min(KP_FWD_SETS_GEN, 4), fused_mfma.hip:1620 (per-DoF lists, r_u streamed): loop :1885-1886
    "fused_fwd_gen_ru0": 6,     # KP_FWD_SETS_GEN, fused_mfma.hip:53 (per-DoF lists, r_u = 0): loop :1885-1886
    "fused_fsc": 4,             # KP_FSC_SETS, fused_mfma.hip:57: state wave :2098-2108 (t + 4 <= T), cost wave :2238-2252 (t + 3 <= T)
    "fused_ring": 2,            # the 2 FPC_BUF slots of the consumer / helper ring, fused_mfma.hip:1410 (slot t & 1, :564, :1354)
    "tiled_fwd": 2,             # KP_FT_SETS, tiled_mfma.hip:23: NS :1179, preload :1193, request :1220, pair loop :1397-1398
    "interp": 16,               # INTERP_TT, elementwise.hip:433: steps per block (:441-442)
    "cost": 4,                  # COST_TT, elementwise.hip:494: steps per block (:505-506)
}
# where each size is written: (file, pattern with one group, or a callable on the file's defines)
_SOURCES = {
    "ric_t1": ("riccati_mfma.hip", r"^#define KP_RIC_SETS (\d+)"),
    "fwd_t1": ("forward_mfma.hip", r"^\s*Tiles S\[(\d+)\];"),
    "fused_fwd_uni": ("fused_mfma.hip", r"^#define KP_FWD_SETS (\d+)"),
    "fused_fwd_gen_ru0": ("fused_mfma.hip", r"^#define KP_FWD_SETS_GEN (\d+)"),
    "fused_fsc": ("fused_mfma.hip", r"^#define KP_FSC_SETS (\d+)"),
    "fused_ring": ("fused_mfma.hip", r"^#define FPC_FLAG \(FPC_RING \+ (\d+) \* FPC_BUF"),
    "tiled_fwd": ("tiled_mfma.hip", r"^#define KP_FT_SETS (\d+)"),
    "interp": ("elementwise.hip", r"^#define INTERP_TT (\d+)"),
    "cost": ("elementwise.hip", r"^#define COST_TT (\d+)"),
}
# the loops whose group is a block of independent steps (one thread block each), not a pipelined body: a block's only
# horizon-dependent code is min(TT, T - t0), so the block edges are held (T below, one short of, equal to and one above a block; the
# last is the default T = 17 of tests/_shapes.py for INTERP_TT = 16), not every residue
BLOCK_LOOPS = ("interp",)

H = (2, 3, 4, 5, 6, 7, 8, 9)
H_RAGGED = (4, 5, 6, 7, 8, 9)                  # at T <= 3 bisect_keypoints gives every DoF the list (0, T-1): no per-DoF set
H_RAGGED6 = tuple(range(4, 14))                # every residue mod 6 below and above one full group
H_BLOCK = (15, 16)
H_LAYOUT = (2, 5, 6)                           # min_N = 4: one segment up to T = 5, a last segment of one step at T = 6
W1 = {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}


def parsed_groups(csrc=CSRC):
    """GROUPS as the sources have it (fused_fwd_gen: the expression of fused_mfma.hip:1620 on the parsed define)."""
    out = {}
    for loop, (name, pat) in _SOURCES.items():
        found = re.findall(pat, open(os.path.join(csrc, name)).read(), re.M)
        assert len(found) == 1, (loop, name, pat, found)
        out[loop] = int(found[0])
    text = open(os.path.join(csrc, "fused_mfma.hip")).read()
    m = re.search(r"constexpr int NS = UNI \? KP_FWD_SETS : \(RU0 \|\| KP_FWD_SETS_GEN < (\d+)\) \? KP_FWD_SETS_GEN : (\d+);", text)
    assert m and m.group(1) == m.group(2), "fused_mfma.hip: NS of forward_fused_body"
    out["fused_fwd_gen"] = min(out["fused_fwd_gen_ru0"], int(m.group(2)))
    return out


def loops_of(c, n_simd):
    """The loops of GROUPS one case runs, from the instantiation keys tests/_shapes.dispatch gives it."""
    d = S.dispatch(c["dof"], c["m"], c["nr"], c["T"], c["n_alpha"], c["batch"], n_simd, c["flags"], c["env"], c["rx_const"], True,
                   c["uniform"])
    bwd, fwd = d["bwd"], d["fwd"]
    out = set()
    if bwd[0] == "t1_bwd":
        out.add("ric_t1")
    if bwd[0] == "fused_bwd" and bwd[3] == "pairh":
        out.add("fused_ring")
    if fwd[0] == "t1_fwd":
        out.add("fwd_t1")
    if fwd[0] == "fused_fwd":
        if fwd[3] != "w1":
            out.add("fused_fsc")
        else:                                           # (r_u = 0 exactly where the case's r_x is the task's constant: _shape_run._problem)
            out.add("fused_fwd_uni" if c["uniform"] else "fused_fwd_gen_ru0" if c["rx_const"] else "fused_fwd_gen")
    if fwd[0] == "tiled_fwd" and fwd[2] == "-" and fwd[3] > 0:      # NS = KP_FT_SETS where NCL > 0 && !A6, tiled_mfma.hip:1179
        out.add("tiled_fwd")
    if "fused" not in d["variants"][0]:                  # _shape_run._backward: the materialising stages
        out.add("interp")
        if not d["variants"][0].endswith("_a6"):
            out.add("cost")
    return out


# form -> (dof, m, nr, flags, env, rx_const, uniform, horizons, the variants _shapes.dispatch must give)
def _forms():
    f = {}
    for n, m in T1_SHAPES:
        dof, nr = n // 2, 9 if (n, m) == (14, 7) else 4
        f[f"fused_w1_d{dof}"] = (dof, m, nr, FLAG_FUSED, W1, True, True, H, "mfma_f64_t1_fused")
        f[f"t1_d{dof}"] = (dof, m, 4, 0, {}, False, True, H, "mfma_f64_t1")
        # per-DoF lists: the general one-wave forward with four sets behind the pair backward, the triple behind the pair
        # forward (what "4" runs on a per-DoF set at 4 x batch <= #SIMDs, plan_forward_fused, fused_mfma.hip:2342-2343) ...
        f[f"fused_ragged_stream_d{dof}"] = (dof, m, 4, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "5", "KPILQR_FUSED_FWD_WAVES": "1"}, False, False,
                                            H_RAGGED, "mfma_f64_t1_fused")
        f[f"fused_ragged_rxc_d{dof}"] = (dof, m, 4, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "0", "KPILQR_FUSED_FWD_WAVES": "4"}, True, False,
                                         H_RAGGED6, "mfma_f64_t1_fused")
    for dof, m in ((7, 7), (2, 1)):
        nr = 9 if dof == 7 else 4
        f[f"fused_w1_triple_d{dof}"] = (dof, m, nr, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "3"}, False, True, H,
                                        "mfma_f64_t1_fused")
        f[f"fused_pair_d{dof}"] = (dof, m, nr, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "5", "KPILQR_FUSED_FWD_WAVES": "4"}, True, True, H,
                                   "mfma_f64_t1_fused")
        # ... and the general one-wave forward with r_u = 0, the only form with six sets (forced: "1")
        f[f"fused_ragged_rxc_w1_d{dof}"] = (dof, m, 4, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "0", "KPILQR_FUSED_FWD_WAVES": "1"}, True, False,
                                            H_RAGGED6, "mfma_f64_t1_fused")
    for dof, m, envs in ((9, 5, ("uw", "no_uw", "no_fsc", "a6")), (19, 8, ("uw", "a6")), (27, 3, ("uw", "no_uw", "a6"))):
        for e in envs:
            f[f"tiled_{e}_d{dof}"] = (dof, m, 4, FLAG_FUSED if e == "a6" else FLAG_TILED, TILED_ENVS[e], False, True, H,
                                      "mfma_f64_tiled_a6" if e == "a6" else "mfma_f64_tiled")
    f["wide_d12"] = (12, 9, 5, 0, {}, False, True, H, "mfma_f64_wide")
    f["wide_d20"] = (20, 17, 5, 0, {}, False, True, H, "mfma_f64_wide")
    f["generic_d3"] = (3, 2, 2, FLAG_GENERIC, {}, False, True, H, "generic_lds")
    f["generic_d32"] = (32, 7, 4, 0, {}, False, True, H, "generic_lds")
    return f


FORMS = _forms()
BLOCK_FORMS = ("t1_d7", "tiled_uw_d9")
LAYOUT_FORMS = ("fused_w1_d7", "t1_d7", "tiled_uw_d9")


def _hcase(form, T, min_N=4):
    dof, m, nr, flags, env, rxc, uni, _, variant = FORMS[form]
    c = _case(dof, m, nr, flags, env, T=T, rx_const=rxc, uniform=uni, why=form)
    # fused cases alternate the two payload forms by the parity of T
    return dict(c, form=form, min_N=min_N, kp_ordered=bool(flags & FLAG_FUSED) and T % 2 == 1, variant=variant)


def cases():
    out = [_hcase(form, T) for form, spec in FORMS.items() for T in spec[7]]
    out += [_hcase(form, T) for form in BLOCK_FORMS for T in H_BLOCK]
    out += [_hcase(form, T, min_N) for form in LAYOUT_FORMS for min_N in (1, 2) for T in H_LAYOUT]
    return out


def case_id(c):
    env = ",".join(f"{k.replace('KPILQR_', '').lower()}={v}" for k, v in sorted(c["env"].items()))
    return f"{c['form']}-T{c['T']}" + (f"-n{c['min_N']}" if c["min_N"] != 4 else "") + (f"-{env}" if env else "")


# ---- a PD failure pinned to a step (tests/test_gpu_horizons.py::test_failure_position).  Every form streams r_u.
FAIL_FORMS = {
    "fused_w1_d7": (7, 7, 4, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "3"}, "mfma_f64_t1_fused"),
    "fused_w1_d6": (6, 3, 2, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "3"}, "mfma_f64_t1_fused"),
    "fused_pairh_d7": (7, 7, 4, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "5", "KPILQR_FUSED_FWD_WAVES": "4"}, "mfma_f64_t1_fused"),
    "fused_pairh_d5": (5, 3, 3, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "5", "KPILQR_FUSED_FWD_WAVES": "4"}, "mfma_f64_t1_fused"),
    "t1_d7": (7, 7, 4, 0, {}, "mfma_f64_t1"),
    "t1_d2": (2, 1, 2, 0, {}, "mfma_f64_t1"),
    "tiled_uw_d9": (9, 5, 4, FLAG_TILED, TILED_ENVS["uw"], "mfma_f64_tiled"),
    "tiled_no_uw_d27": (27, 3, 4, FLAG_TILED, TILED_ENVS["no_uw"], "mfma_f64_tiled"),
    "tiled_a6_d19": (19, 8, 4, FLAG_FUSED, TILED_ENVS["a6"], "mfma_f64_tiled_a6"),
    "wide_d12": (12, 9, 5, 0, {}, "mfma_f64_wide"),
    "generic_d3": (3, 2, 2, FLAG_GENERIC, {}, "generic_lds"),
}
# both steps of a pair, the terminal step and step 0: every step of T = 2, 3, 5, and the ends and the middle pair of T = 8
FAIL_STEPS = {2: (0, 1), 3: (0, 1, 2), 5: (0, 1, 2, 3, 4), 8: (0, 3, 4, 7)}


def failure_cases():
    out = []
    for form, (dof, m, nr, flags, env, variant) in FAIL_FORMS.items():
        for T, steps in FAIL_STEPS.items():
            for ts in steps:
                c = _case(dof, m, nr, flags, env, T=T, why=form)
                out.append(dict(c, form=form, min_N=4, kp_ordered=bool(flags & FLAG_FUSED) and T % 2 == 1, variant=variant, t_star=ts))
    return out


def failure_id(c):
    return f"{c['form']}-T{c['T']}-t{c['t_star']}"


def failing_problem(p, t_star):
    """Problem p (dense residuals) with residual j = nr - 1 turned into a PD failure of trajectory 1 at step t_star and nothing
    else: weights -1e3, the residual and its Jacobians zero everywhere but r_u[1, t_star, j], a unit row -- l_uu of that step
    gets -2e3 v v', every other step's cost is that of the residuals 0 .. nr - 2."""
    import numpy as np
    q = dict(p)
    j = p["nr"] - 1
    for key in ("w_run", "w_term", "r", "r_x", "r_u"):
        q[key] = p[key].copy()
    row = p["r_u"][1, t_star, j].copy()
    q["w_run"][j] = q["w_term"][j] = -1e3
    q["r"][:, :, j] = 0.0
    q["r_x"][:, :, j] = 0.0
    q["r_u"][:, :, j] = 0.0
    q["r_u"][1, t_star, j] = row / np.linalg.norm(row)
    return q
