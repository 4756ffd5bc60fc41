"""The kernel dispatch of libkpilqr, restated in Python: which kernel family and which compiled instantiation a context of a
given shape runs, the hand-written list of instantiations the library compiles, and a chooser that names, for every
instantiation, the smallest and the largest problem that reaches it.  tests/test_shape_table.py checks the table against itself
(no GPU); tests/test_gpu_shapes.py runs every case and asserts the variant the table predicts.

File:line citations are to trajoptkp_amd/csrc.  n = 2 dof; T1_SHAPES are the (n, m) pairs of the one-tile kernels."""

FLAG_GENERIC, FLAG_TILED, FLAG_FUSED = 1, 2, 4          # include/kpilqr.h:75-77
T1_SHAPES = ((14, 7), (4, 1), (12, 3), (10, 3))        # KP_T1_SHAPES, mfma_common.h:174
BIGOFF = 0x40000000                                     # fused_mfma.hip:44
TILE, TPAD = 256, 272                                   # KP_TILE, KP_TPAD, mfma_common.h:20-21
LDS_MAX = 160 * 1024                                    # the LDS bound of the tiled and generic backward sweeps
FSC_REC_BYTES_MAX = 0x7fffff00                          # KP_FSC_REC_BYTES_MAX, tiled_mfma.hip:27: one trajectory's records in one descriptor
ENV_KEYS = ("KPILQR_FUSED_WAVES", "KPILQR_FUSED_FWD_WAVES", "KPILQR_TILED_NT_MIN", "KPILQR_TILED_A6", "KPILQR_TILED_UW",
            "KPILQR_TILED_FSC")


def _env(env, key, default):                            # read_tuning_from_env, kpilqr_api.cpp
    v = (env or {}).get(key)
    return default if v is None or v == "" else int(v)


def _cdiv(a, b):                                        # C's int division (truncates toward zero)
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def rec_stride(n, m):                                   # RecLayout::stride, common.h:29-37 (doubles; the record padded to 16)
    return (2 * n * n + n * m + n + m * m + m + 15) & ~15


def tiled_nt(n, nt_min=0):                              # tiled_nt, tiled_mfma.hip:562 (wide_nt, tiled_wide.hip:413, is the same)
    return max((n + 1 + 15) // 16, 2, nt_min)


def backward_col_lds_bytes(nt):                         # tiled_mfma.hip:554
    return 8 * ((2 * nt * nt + 7 * nt) * TILE + max(nt * nt * TPAD, 832))


def generic_lds_bytes(n, m):                            # backward_generic_lds_bytes, generic.hip:93
    return 8 * (2 * n * n + 4 * m * n + 5 * m * m + 2 * n + 4 * m + m + 2)


def fused_supported(n, m, nr, dof, T, n_alpha):         # fused_mfma.hip:2177
    return (n, m) in T1_SHAPES and 1 <= nr <= 16 and m <= dof and n_alpha <= 16 and T * dof * (6 * n + 2) * 8 < BIGOFF


def backward_tiled_supported(n, m, nt_min=0):           # tiled_mfma.hip:572
    nt = tiled_nt(n, nt_min)
    return 2 <= nt <= 4 and 1 <= m <= 8 and backward_col_lds_bytes(nt) <= LDS_MAX


def forward_t1_supported(n, m, n_alpha):                # forward_mfma_supported, forward_mfma.hip:159
    return n + 2 <= 16 and m <= 8 and n_alpha <= 16 and n >= 2


def forward_tiled_supported(n, m, n_alpha, nt_min=0):   # tiled_mfma.hip:1734
    return 2 <= tiled_nt(n, nt_min) <= 4 and m <= 16 and n_alpha <= 16


def backward_wide_supported(n, m, nt_min=0):            # tiled_wide.hip:421
    return 2 <= tiled_nt(n, nt_min) <= 4 and 8 < m <= 32


def forward_wide_supported(n, m, n_alpha, nt_min=0):    # tiled_wide.hip:649
    return 2 <= tiled_nt(n, nt_min) <= 4 and 16 < m <= 32 and n_alpha <= 16


def select_variants(dof, m, nr, T, n_alpha, batch, flags, env=None):
    """select_variants (kpilqr_api.cpp): (backward variant, forward variant), or None where kpilqr_create refuses the
    shape with KPILQR_ERR_ARG (the generic backward sweep's LDS, its last check)."""
    n = 2 * dof
    nt_min = _env(env, "KPILQR_TILED_NT_MIN", 0)
    generic, force_tiled = bool(flags & FLAG_GENERIC), bool(flags & FLAG_TILED)
    bv = ("mfma_f64_t1" if not generic and not force_tiled and (n, m) in T1_SHAPES            # riccati_mfma.hip:342
          else "mfma_f64_tiled" if not generic and backward_tiled_supported(n, m, nt_min)
          else "mfma_f64_wide" if not generic and backward_wide_supported(n, m, nt_min) else "generic_lds")
    fv = ("mfma_f64_t1" if not generic and not force_tiled and forward_t1_supported(n, m, n_alpha)
          else "mfma_f64_tiled" if not generic and forward_tiled_supported(n, m, n_alpha, nt_min)
          else "mfma_f64_wide" if not generic and forward_wide_supported(n, m, n_alpha, nt_min) else "generic_lds")
    fused = bool(flags & FLAG_FUSED) and not generic and not force_tiled and fused_supported(n, m, nr, dof, T, n_alpha)
    if fused:
        bv = fv = "mfma_f64_t1_fused"
    elif flags & FLAG_FUSED and bv == fv == "mfma_f64_tiled":           # (the tiled_a6 choice)
        a6 = _env(env, "KPILQR_TILED_A6", -1)
        if nr <= 16 and (a6 != 0 if a6 >= 0 else (tiled_nt(n, nt_min) == 4 and batch >= 96)):
            bv = fv = "mfma_f64_tiled_a6"
    if bv == "generic_lds" and generic_lds_bytes(n, m) > LDS_MAX:
        return None
    return bv, fv


def rv2_ncr(nr):
    """4-row chunks of the relabelled residual rows of the one-wave fused sweeps with a constant r_x and r_u = 0 (RV2B,
    fused_mfma.hip:283; RV2 in the forward sweep, :1388-1411): registers 0, 1 of a lane hold residuals 0 .. 7, 2, 3 hold 8 .. 15."""
    return 4 if nr > 9 else 3 if nr > 8 else 2 if nr > 1 else 1


def dispatch(dof, m, nr, T, n_alpha, batch, n_simd, flags, env=None, rx_const=False, ru_zero=True, uniform=True):
    """What one iteration of a context launches.  Returns None where kpilqr_create refuses, else a dict with
      variants: (backward, forward) variant names (kpilqr_backward_variant / kpilqr_forward_variant)
      bwd, fwd: the instantiation keys of the sweeps (tuples, first element the family; the keys of COMPILED)
      extra:    further keys the launch covers (the RV2 residual chunk count of the one-wave fused sweeps)
      launch:   substrings kpilqr_last_launch must contain, (backward, forward)."""
    sel = select_variants(dof, m, nr, T, n_alpha, batch, flags, env)
    if sel is None:
        return None
    bv, fv = sel
    n = 2 * dof
    nt = tiled_nt(n, _env(env, "KPILQR_TILED_NT_MIN", 0))
    uw = _env(env, "KPILQR_TILED_UW", -1)
    excl = "excl" if batch <= n_simd else "plain"       # riccati_mfma.hip:351, forward_mfma.hip:168, FusedLaunch::excl, fused_mfma.hip:2212, 2232
    ncz, ncu = (n + 2 + 3) // 4, (m + 3) // 4
    out = dict(variants=(bv, fv), extra=(), launch=(bv, fv))
    if bv == "mfma_f64_t1_fused":
        f = _env(env, "KPILQR_FUSED_WAVES", 0)
        bform = f if f in (1, 5) else (5 if 2 * batch <= n_simd else 1)           # plan_backward_fused, fused_mfma.hip:2201-2205
        f = _env(env, "KPILQR_FUSED_FWD_WAVES", 0)
        fform = f if f in (1, 3, 4) else (4 if 2 * batch <= n_simd else 1)        # plan_forward_fused, :2223-2227
        out["bwd"] = ("fused_bwd", n, m, "w1", excl) if bform == 1 else ("fused_bwd", n, m, "pairh", "-")
        if fform == 4:                                  # the uniform pair; per-DoF lists run the triple or w1 behind it (waves_ragged, :2228)
            behind = 3 if 4 * batch <= n_simd else 1
            fform_ran = 4 if uniform else behind
        else:
            fform_ran = fform
        fname = {1: "w1", 3: "triple", 4: "pair"}[fform_ran]
        out["fwd"] = ("fused_fwd", ncz, ncu, fname, excl if fname == "w1" else "-")
        rxc = rx_const and ru_zero
        if rxc and bform == 1:
            out["extra"] = (("fused_rv2", n, m, rv2_ncr(nr)),)
        # kpilqr_last_launch (kpilqr_api.cpp): ":w1:" / ":pairh:" / ":pair:" / ":triple:" (the forward pair reports the form
        # that ran on this set)
        out["launch"] = (bv + (":w1:" if bform == 1 else ":pairh:"), fv + ":" + {1: "w1", 3: "triple", 4: "pair"}[fform_ran] + ":")
        return out
    if bv == "mfma_f64_t1":
        out["bwd"] = ("t1_bwd", n, m, excl)             # launch_backward_mfma, riccati_mfma.hip:357
    elif bv.startswith("mfma_f64_tiled"):
        a6 = bv.endswith("_a6")
        M = 7 if m == 7 else 1 if m == 1 else 8         # launch_backward_tiled, tiled_mfma.hip:1047-1053
        if nt <= 3 and not a6 and uw != 0:              # launch_bt, :1041-1044
            rows = n + 1 - 16 * (nt - 1)                # launch_bt_uw, :1000-1010
            ncl = 4 if rows >= 16 else max(_cdiv(rows + 3, 4), 1)
            out["bwd"] = ("tiled_bwd", M, nt, ncl, "uw")
        else:
            ncl = 0
            if nt == 4 and uw != 0:                     # launch_bt2, :1025-1037
                rows = n + 1 - 16 * (nt - 1)
                ncl = 4 if rows >= 16 else _cdiv(rows + 3, 4)
            out["bwd"] = ("tiled_bwd", M, nt, ncl, "a6" if a6 else "col")
    elif bv == "mfma_f64_wide":
        out["bwd"] = ("wide_bwd", nt, 2 if m > 16 else 1)   # launch_backward_wide, tiled_wide.hip:438-444
    else:
        out["bwd"] = ("generic_bwd",)
    if fv == "mfma_f64_t1":                             # launch_forward_mfma, forward_mfma.hip:174-204
        out["fwd"] = ("t1_fwd", max(ncz, 2), min(ncu, 2), excl)
    elif fv.startswith("mfma_f64_tiled"):
        a6 = fv.endswith("_a6")
        fsc = _env(env, "KPILQR_TILED_FSC", -1)
        # forward_tiled_sc_selected, tiled_mfma.hip:1814-1825: a horizon whose records outgrow the form's one descriptor per trajectory
        # runs the general form, whatever KPILQR_TILED_FSC says
        sc = (nt == 2 and not a6 and m <= 8 and T * rec_stride(n, m) * 8 <= FSC_REC_BYTES_MAX
              and (fsc != 0 if fsc >= 0 else 2 * nt * batch <= n_simd))
        rows = n + 2 - 16 * (nt - 1)
        if sc:                                          # launch_ft_sc, :1771-1779
            ncl = 4 if rows >= 16 else 1 if rows < 1 else _cdiv(rows + 3, 4)
            out["fwd"] = ("tiled_fwd_sc", ncl, ncu)
            out["launch"] = (out["launch"][0], fv + ":state_cost_waves")
        else:                                           # launch_ft2, :1751-1764
            ncl = (4 if rows >= 16 else max(_cdiv(rows + 3, 4), 1)) if uw != 0 else 0
            out["fwd"] = ("tiled_fwd", nt, "a6" if a6 else "-", ncl)
    elif fv == "mfma_f64_wide":
        out["fwd"] = ("wide_fwd", nt)                   # launch_forward_wide, tiled_wide.hip:668-675
    else:
        out["fwd"] = ("generic_fwd",)
    return out


def _compiled():
    """The instantiations the library compiles, by hand from the launchers (not derived from dispatch)."""
    keys = []
    for n, m in T1_SHAPES:
        keys += [("t1_bwd", n, m, e) for e in ("excl", "plain")]                       # launch_bm, riccati_mfma.hip:347-362
        keys += [("fused_bwd", n, m, "w1", e) for e in ("excl", "plain")]              # launch_bf_kernel ... launch_backward_fused, fused_mfma.hip:2237-2281
        keys += [("fused_bwd", n, m, "pairh", "-")]                                    # launch_bph_kernel ... launch_backward_fused_pair, :2287-2322
        keys += [("fused_rv2", n, m, ncr) for ncr in (1, 2, 3, 4)]                     # :283
    keys += [("t1_fwd", ncz, ncu, e) for ncz in (2, 3, 4) for ncu in (1, 2) for e in ("excl", "plain")]   # launch_fm, forward_mfma.hip:164-178
    for ncz, ncu in ((4, 2), (2, 1), (4, 1), (3, 1)):                                  # KP_FWD_SHAPES, fused_mfma.hip:2387 (launch_ff_pair, _triple, _w1: 2418-2448)
        keys += [("fused_fwd", ncz, ncu, "w1", e) for e in ("excl", "plain")]
        keys += [("fused_fwd", ncz, ncu, f, "-") for f in ("pair", "triple")]
    for M in (1, 7, 8):                                                                # tiled_mfma.hip:1047-1053
        keys += [("tiled_bwd", M, nt, ncl, "uw") for nt in (2, 3) for ncl in (1, 2, 3, 4)]          # :1003-1008
        keys += [("tiled_bwd", M, 4, ncl, f) for ncl in (1, 2, 3, 4) for f in ("col", "a6")]      # :1031-1036
        keys += [("tiled_bwd", M, nt, 0, f) for nt in (2, 3, 4) for f in ("col", "a6")]           # :1037
    keys += [("tiled_fwd", nt, a6, ncl) for nt in (2, 3, 4) for a6 in ("-", "a6") for ncl in (0, 1, 2, 3, 4)]   # :1760-1765
    keys += [("tiled_fwd_sc", ncl, ncu) for ncu in (1, 2) for ncl in (1, 2, 3, 4)]                       # KP_SC, :1776
    keys += [("wide_bwd", nt, mt) for nt in (2, 3, 4) for mt in (1, 2)]                                  # tiled_wide.hip:441-442
    keys += [("wide_fwd", nt) for nt in (2, 3, 4)]                                                       # tiled_wide.hip:671-673
    keys += [("generic_bwd",), ("generic_fwd",)]
    return keys


COMPILED = _compiled()


def case_keys(case, n_simd):
    """The instantiation keys one case (a dict: dof, m, nr, T, n_alpha, batch, flags, env, rx_const, uniform) reaches."""
    d = dispatch(case["dof"], case["m"], case["nr"], case["T"], case["n_alpha"], case["batch"], n_simd, case["flags"],
                 case.get("env"), case.get("rx_const", False), True, case.get("uniform", True))
    return () if d is None else (d["bwd"], d["fwd"]) + tuple(d["extra"])


def _case(dof, m, nr, flags, env=None, T=17, batch=2, n_alpha=6, rx_const=False, uniform=True, why=""):
    return dict(dof=dof, m=m, nr=nr, T=T, batch=batch, n_alpha=n_alpha, flags=flags, env=dict(env or {}), rx_const=rx_const,
                uniform=uniform, why=why)


# the environments that reach the forms of the tiled families (read at kpilqr_create)
TILED_ENVS = {"uw": {}, "a6": {"KPILQR_TILED_A6": "1"}, "no_uw": {"KPILQR_TILED_UW": "0", "KPILQR_TILED_A6": "0"},
              "no_uw_a6": {"KPILQR_TILED_UW": "0", "KPILQR_TILED_A6": "1"}, "no_fsc": {"KPILQR_TILED_FSC": "0"}}


def chooser(n_simd):
    """For every compiled key of the tiled, wide and t1 families, the smallest and the largest shape that reaches it (over dof
    1 .. 31, every m the family takes), found by running dispatch over the grid.  Returns {key: [case, ...]}."""
    found = {}
    grid = []
    for dof in range(1, 32):
        for m in range(1, 33):
            for flags, envs in ((FLAG_TILED, ("uw", "no_uw", "no_fsc")), (FLAG_TILED | FLAG_FUSED, ("a6", "no_uw_a6")), (0, ("uw",))):
                for e in envs:
                    grid.append((dof, m, flags, e))
    for dof, m, flags, e in grid:
        c = _case(dof, m, 3, flags, TILED_ENVS[e], why=f"chooser:{e}")
        if flags & FLAG_FUSED:                          # (fused on a tiled shape: a6 needs both sweeps tiled)
            d = select_variants(dof, m, 3, c["T"], 6, 2, flags, c["env"])
            if d is None or not d[0].endswith("_a6"):
                continue
        for key in case_keys(c, n_simd):
            if key[0].startswith(("fused", "generic")):
                continue
            lo_hi = found.setdefault(key, [None, None])
            size = (2 * dof, m)
            if lo_hi[0] is None or size < (2 * lo_hi[0]["dof"], lo_hi[0]["m"]):
                lo_hi[0] = c
            if lo_hi[1] is None or size > (2 * lo_hi[1]["dof"], lo_hi[1]["m"]):
                lo_hi[1] = c
    return {k: [c for i, c in enumerate(v) if c is not None and (i == 0 or c is not v[0])] for k, v in found.items()}


def cases(n_simd):
    """The cases of tests/test_gpu_shapes.py that run at batch 2 .. 3 (the batch-boundary cases are built there from n_simd).
    Every case carries `why`, the group it belongs to."""
    out = []
    # fused one-tile sweeps: every RV2 residual chunk count at its smallest and largest nr on every shape, one wave (rxc) ...
    for n, m in T1_SHAPES:
        for nr in (1, 2, 8, 9, 10, 16):
            out.append(_case(n // 2, m, nr, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}, rx_const=True,
                             why="fused_rv2"))
    for nr in (13, 15):
        out.append(_case(7, 7, nr, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}, rx_const=True, why="fused_rv2"))
    # ... and the wave forms, with r_x streamed and constant, on uniform and per-DoF lists
    for n, m in T1_SHAPES:
        for nr in (1, 16):
            for bw, fw, rxc, uni in (("5", "4", True, True), ("1", "3", False, True), ("5", "1", False, False), ("0", "4", True, False)):
                out.append(_case(n // 2, m, nr, FLAG_FUSED, {"KPILQR_FUSED_WAVES": bw, "KPILQR_FUSED_FWD_WAVES": fw}, rx_const=rxc,
                                 uniform=uni, why="fused_forms"))
    # the tiled, wide and one-tile families: the chooser's smallest and largest shape of every key
    seen = set()
    for key, cs in sorted(chooser(n_simd).items(), key=lambda kv: str(kv[0])):
        for c in cs:
            sig = (c["dof"], c["m"], c["flags"], tuple(sorted(c["env"].items())))
            if sig not in seen:
                seen.add(sig); out.append(c)
    # m on both sides of the M (1 | 7 | 8-padded) and NCU (m <= 4 | 5 .. 8) switches, every tiled form, two and three tiles
    for dof in (9, 19):
        for m in (1, 4, 5, 8):
            for e in ("uw", "no_uw", "no_fsc"):
                out.append(_case(dof, m, 4, FLAG_TILED, TILED_ENVS[e], why="tiled_m"))
            out.append(_case(dof, m, 4, FLAG_FUSED, TILED_ENVS["a6"], why="tiled_m"))
    # wide: NT 2, 3, 4 at m = 9, 16, 17, 32
    for dof in (12, 20, 28):
        for m in (9, 16, 17, 32):
            out.append(_case(dof, m, 5, 0, why="wide"))
    # n_alpha 1, 7, 16 on every forward family (17: the generic fallback)
    for dof, m, flags, env in ((7, 7, 0, {}), (7, 7, FLAG_FUSED, {"KPILQR_FUSED_FWD_WAVES": "1"}), (7, 7, FLAG_FUSED, {"KPILQR_FUSED_FWD_WAVES": "3"}),
                               (7, 7, FLAG_FUSED, {"KPILQR_FUSED_FWD_WAVES": "4"}), (12, 7, 0, {}), (12, 7, 0, TILED_ENVS["no_fsc"]),
                               (12, 7, FLAG_FUSED, TILED_ENVS["a6"]), (20, 7, 0, {}), (20, 21, 0, {})):
        for na in (1, 7, 16, 17):
            out.append(_case(dof, m, 4, flags, env, n_alpha=na, rx_const=bool(flags), why="n_alpha"))
    # fallbacks: nr = 17 leaves the fused and the a6 forms; m > dof is never fused; dof = 32 and the generic LDS bound
    out.append(_case(7, 7, 17, FLAG_FUSED, rx_const=True, why="fallback"))
    out.append(_case(12, 7, 17, FLAG_FUSED, TILED_ENVS["a6"], why="fallback"))
    out.append(_case(2, 3, 2, FLAG_FUSED, why="fallback"))
    out.append(_case(5, 7, 4, FLAG_FUSED, why="fallback"))
    out.append(_case(32, 7, 4, 0, why="fallback"))
    out.append(_case(GENERIC_MAX_DOF_M7, 7, 4, 0, T=5, why="fallback"))
    out.append(_case(GENERIC_MAX_DOF_M7 + 1, 7, 4, 0, T=5, why="refused"))
    # one case per family with T >= 129: the Newton-Schulz refresh and the PD stride (100) crossed
    for dof, m, flags, env in ((7, 7, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}), (7, 7, FLAG_FUSED, {}),
                               (3, 2, 0, {}), (14, 5, FLAG_TILED, {}), (21, 8, FLAG_FUSED, TILED_ENVS["a6"]), (27, 3, FLAG_TILED, {}),
                               (16, 17, 0, {}), (18, 12, 0, {})):
        out.append(_case(dof, m, 4, flags, env, T=131, rx_const=bool(flags & FLAG_FUSED), why="long"))
    return out


def generic_max_dof(m):
    """The largest dof whose generic backward sweep fits the LDS bound (select_variants in kpilqr_api.cpp, generic.hip:93)."""
    dof = 1
    while generic_lds_bytes(2 * (dof + 1), m) <= LDS_MAX:
        dof += 1
    return dof


GENERIC_MAX_DOF_M7 = generic_max_dof(7)



def batch_cases(n_simd):
    """Both sides of the batch bounds (built in tests/test_gpu_shapes.py with synth.tile_problem): n_simd and n_simd + 1 for the
    excl / plain pairs of the one-tile and the one-wave fused sweeps (every shape, constant r_x), n_simd / 4 and one more for
    the tiled state / cost forward (2 NT batch <= n_simd, NT = 2)."""
    out = []
    for n, m in T1_SHAPES:
        for b in (n_simd, n_simd + 1):
            out.append(_case(n // 2, m, 4, 0, batch=b, why="batch"))
            out.append(_case(n // 2, m, 9 if n == 14 else 4, FLAG_FUSED, batch=b, rx_const=True, why="batch"))
    for dof, m in ((2, 5), (4, 6)):                     # the plain one-tile forward with two control chunks (its backward is tiled)
        out.append(_case(dof, m, 4, 0, batch=n_simd + 1, why="batch"))
    for b in (n_simd // 4, n_simd // 4 + 1):
        out.append(_case(12, 7, 4, 0, batch=b, why="batch"))
    return out
