"""Batches whose device buffers need offsets beyond 32 bits: the case table of tests/test_gpu_large_offsets.py, the bytes of every
device buffer of a case from the sources' own formulas, where a truncated offset would land, and the largest horizon every sweep
form can address inside ONE trajectory.  tests/test_large_offset_table.py checks the table (no GPU).

Three thresholds are separate failure modes of one missing cast:
  bytes31   2^31 bytes      an `int` byte offset, or a buffer-descriptor offset from the buffer's base
  bytes32   2^32 bytes      an `unsigned` byte offset
  elems31   2^31 elements   an `int` element index such as (b * T + t) * stride   (16 GiB of doubles)

A case is UNIQ distinct trajectories (seeds synth.seed_for(config_id, 0 .. UNIQ-1)) replicated `reps` times along the batch: trajectory
b carries seed b mod UNIQ.  UNIQ is an odd prime and the horizons are primes, so no power-of-two truncation maps a (trajectory, step)
onto a replica of itself at the same step: aliased() computes where every truncation of every checked offset lands and says so.
The horizons stay in the hundreds -- the batch carries the offset --, key-points sit on four steps of every trajectory, and the host
arrays are those of the UNIQ trajectories: the per-trajectory inputs are tiled on the device (Engine.device_array).

File:line citations are to trajoptkp_amd/csrc."""
import os
import re

import numpy as np

import _shapes as S
from _shapes import FLAG_FUSED, FLAG_GENERIC, FLAG_TILED, TILED_ENVS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trajoptkp_amd", "csrc")
UNIQ = 7
CAP = 48 << 30                          # the most device memory a case may plan for (a condition, not a measurement)
HEADROOM = 8 << 30                      # what the GPU test wants free beyond the table size (torch's temporaries, the runtime)
THRESHOLDS = {"bytes31": 2 ** 31, "bytes32": 2 ** 32, "elems31": 2 ** 31}
N_ALPHA = 2                             # U_alpha of the whole batch comes down: two step sizes keep it at a gigabyte
CONFIG_ID, CONFIG_ID_LISTED = 21, 22    # the seeds of the batch, and the fresh ones of the listed trajectories
W1 = {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}


def _lc(name, families, dof, m, nr, T, reps, flags, env=None, payload="jobs", rx="step", uniform=True, k_carrier=None, listed=False):
    """payload: "jobs" | "kp_ordered" (kpilqr_upload_fd | kpilqr_upload_fd_kp).  rx: "step" -- dense per-step r_x and r_u, tiled on the
    device -- or "const" (kpilqr_upload_residual_jacobians_const, r_u = 0).  k_carrier: the case of the same kernel template that has
    K past 2^32 bytes where this shape cannot have it under CAP.  listed: the partial calls run on this context too."""
    return dict(name=name, families=tuple(families), dof=dof, m=m, nr=nr, T=T, reps=reps, batch=reps * UNIQ, flags=flags,
                env=dict(env or {}), payload=payload, rx=rx, rx_const=rx == "const", uniform=uniform, n_alpha=N_ALPHA,
                k_carrier=k_carrier, listed=listed, why="large")


# The sweep families of the library and the cases that carry them.  Sizes (doubles per step): one-tile (14, 7) records 560, K 98;
# two-tile (8, 8) through FLAG_TILED 272, 64; three-tile (32, 8) 2416, 256; four-tile (62, 7) 8240, 434; wide (10, 9) 400, 90 and
# (18, 17) 1280, 306; the fused sweeps' per-step r_x at nr = 16: 224.
CASES = [
    # materialising one tile, the plain (not exclusive) kernels; the key-point ordered payload, so that the listed route has one
    _lc("t1_plain", ["t1_plain"], 7, 7, 2, 523, 1501, 0, payload="kp_ordered", listed=True),
    # fused one wave: the raw payload on a uniform set, per-step r_x on per-DoF lists (job lists: the column store), constant r_x
    _lc("fused_w1_raw_uni", ["fused_w1"], 7, 7, 16, 523, 2619, FLAG_FUSED, W1, payload="kp_ordered", listed=True),
    _lc("fused_w1_ragged", ["fused_w1"], 7, 7, 16, 523, 2619, FLAG_FUSED, W1, uniform=False),
    _lc("fused_w1_rxc", ["fused_w1"], 7, 7, 9, 523, 1501, FLAG_FUSED, W1, payload="kp_ordered", rx="const"),
    # the fused wave forms, which the environment selects at any batch: consumer / helper pair + state / cost pair, one wave + triple
    _lc("fused_pairh_pair", ["fused_waves"], 7, 7, 16, 523, 2619, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "5", "KPILQR_FUSED_FWD_WAVES": "4"},
        payload="kp_ordered"),
    _lc("fused_w1_triple", ["fused_waves"], 7, 7, 16, 523, 2619, FLAG_FUSED, {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "3"}),
    # tiled, the uw backward form at two tiles under both forward forms (the general one, the state / cost waves forced) ...
    _lc("tiled_uw_2_fwd", ["tiled_uw", "tiled_fwd"], 4, 8, 2, 523, 2292, FLAG_TILED, TILED_ENVS["no_fsc"]),
    _lc("tiled_uw_2_fsc", ["tiled_uw", "tiled_fwd"], 4, 8, 2, 523, 2292, FLAG_TILED, {"KPILQR_TILED_FSC": "1"}),
    # ... and at three tiles, the smallest three-tile shape: K past 2^32 bytes takes 40 GB of records there, which the cap still holds
    _lc("tiled_uw_3", ["tiled_uw"], 16, 8, 2, 509, 589, FLAG_TILED),
    # four tiles, col and a6 (K past 2^32 bytes: 81 GB of records); the same templates at two tiles carry K
    _lc("tiled_col_4", ["tiled_col_a6"], 31, 7, 2, 509, 74, 0, k_carrier="tiled_col_2"),
    _lc("tiled_a6_4", ["tiled_col_a6"], 31, 7, 2, 509, 74, FLAG_FUSED, TILED_ENVS["a6"], k_carrier="tiled_a6_2"),
    _lc("tiled_col_2", ["tiled_col_a6"], 4, 8, 2, 523, 2292, FLAG_TILED, TILED_ENVS["no_uw"]),
    _lc("tiled_a6_2", ["tiled_col_a6"], 4, 8, 2, 523, 2292, FLAG_TILED | FLAG_FUSED, TILED_ENVS["a6"]),
    # wide: one and two control tiles (m = 9: the tiled forward sweep takes it; m = 17: the wide one)
    _lc("wide_m9", ["wide"], 5, 9, 2, 523, 1630, 0),
    _lc("wide_m17", ["wide"], 9, 17, 2, 523, 480, 0),
    _lc("generic", ["generic"], 7, 7, 2, 523, 1501, FLAG_GENERIC),
]
BY_NAME = {c["name"]: c for c in CASES}
FAMILIES = ("t1_plain", "fused_w1", "fused_waves", "tiled_uw", "tiled_col_a6", "tiled_fwd", "wide", "generic")
# (backward variant, forward variant, substrings of the two launch strings) every case must run as
EXPECT = {
    "t1_plain": ("mfma_f64_t1", "mfma_f64_t1", "", ""),
    "fused_w1_raw_uni": ("mfma_f64_t1_fused", "mfma_f64_t1_fused", ":w1:raw:uni", ":w1:uni"),
    "fused_w1_ragged": ("mfma_f64_t1_fused", "mfma_f64_t1_fused", ":w1:", ":w1:"),
    "fused_w1_rxc": ("mfma_f64_t1_fused", "mfma_f64_t1_fused", ":rxc", ":rxc"),
    "fused_pairh_pair": ("mfma_f64_t1_fused", "mfma_f64_t1_fused", ":pairh:", ":pair:"),
    "fused_w1_triple": ("mfma_f64_t1_fused", "mfma_f64_t1_fused", ":w1:", ":triple:"),
    "tiled_uw_2_fwd": ("mfma_f64_tiled", "mfma_f64_tiled", "", ""),
    "tiled_uw_2_fsc": ("mfma_f64_tiled", "mfma_f64_tiled", "", ":state_cost_waves"),
    "tiled_uw_3": ("mfma_f64_tiled", "mfma_f64_tiled", "", ""),
    "tiled_col_4": ("mfma_f64_tiled", "mfma_f64_tiled", "", ""),
    "tiled_a6_4": ("mfma_f64_tiled_a6", "mfma_f64_tiled_a6", "", ""),
    "tiled_col_2": ("mfma_f64_tiled", "mfma_f64_tiled", "", ""),
    "tiled_a6_2": ("mfma_f64_tiled_a6", "mfma_f64_tiled_a6", "", ""),
    "wide_m9": ("mfma_f64_wide", "mfma_f64_tiled", "", ""),
    "wide_m17": ("mfma_f64_wide", "mfma_f64_wide", "", ""),
    "generic": ("generic_lds", "generic_lds", "", ""),
}


def case_id(c):
    return c["name"]


def is_fused(c):
    return EXPECT[c["name"]][0] == "mfma_f64_t1_fused"


# ---- key-points and problems ---------------------------------------------------------------------------------------------------
def kp_lists(c, u, listed=False):
    """The per-DoF key-point times of unique trajectory u: four steps each.  Uniform sets: one list for every DoF (and trajectory);
    per-DoF sets: the two interior key-points move with the DoF and the trajectory.  listed: the lists the listed trajectories get
    from kpilqr_update_keypoints -- five steps, so that the entry ranges of everybody behind them move."""
    T, dof = c["T"], c["dof"]
    if c["uniform"]:                    # synth.keypoint_rows_set_interval at min_N = uniform_min_N: steps 0, min_N, 2 min_N .., T - 1
        min_N = uniform_min_N(c, listed)
        return [[t for t in range(T) if (t < T - 1 and t % min_N == 0) or t == T - 1]] * dof
    out = []
    for d in range(dof):
        a = 1 + (37 * d + 13 * u + (5 if listed else 0)) % (T - 2)
        b = 1 + (101 * d + 29 * u + 211) % (T - 2)
        extra = [1 + (7 * d + 3 * u) % (T - 2)] if listed else []
        out.append(sorted({0, T - 1, a, b, *extra}))
    return out


def uniform_min_N(c, listed=False):
    return c["T"] // 4 + 1 if listed else c["T"] // 3 + 1          # five | four key-points


def problem(c, listed=False):
    """The host problem of a case: UNIQ trajectories (listed: 3, with fresh seeds and lists) from synth.make_problem (uniform sets: FD
    jobs for every column, the controls beyond dof included) or synth.make_ragged_problem (per-DoF lists), with dense per-step residual
    Jacobians (rx "step") or the task's constant selector rows (rx "const", r_u = 0)."""
    from trajoptkp_amd import synth
    task = synth.shape_task(c["dof"], c["m"], c["nr"])
    count = 3 if listed else UNIQ
    config_id = CONFIG_ID_LISTED if listed else CONFIG_ID
    if c["payload"] == "kp_ordered":    # (control columns beyond dof have no slot in a by-entry payload)
        assert c["m"] <= c["dof"]
    if c["uniform"]:
        p = synth.make_problem(task=task, T=c["T"], batch=count, min_N=uniform_min_N(c, listed), dense_residuals=c["rx"] == "step",
                               one_sided_frac=0.1, config_id=config_id)
    else:
        rows = [synth.rows_from_dof_lists(c["dof"], c["T"], kp_lists(c, u, listed)) for u in range(count)]
        p = synth.make_ragged_problem(task, c["T"], rows, config_id=config_id, dense_residuals=c["rx"] == "step", one_sided_frac=0.1)
    lists = [kp_lists(c, u, listed) for u in range(count)]
    offs, times = dof_csr(p)
    assert [list(times[offs[i]:offs[i + 1]]) for i in range(count * c["dof"])] == [l for per in lists for l in per]
    return p


def dof_csr(p):
    from trajoptkp_amd.engine import rows_to_dof_csr
    return rows_to_dof_csr(p["kp_rows"], p["dof"], p["T"])


def tiled_csr(p, reps):
    """The per-DoF CSR of p's trajectories replicated reps times (without walking reps * UNIQ * dof lists)."""
    offs, times = dof_csr(p)
    E = int(offs[-1])
    full = (offs[:-1][None, :].astype(np.int64) + E * np.arange(reps, dtype=np.int64)[:, None]).reshape(-1)
    return np.concatenate([full, [E * reps]]).astype(np.int32), np.tile(times, reps)


def tiled_jobs(p, reps):
    """The FD job lists of p replicated reps times: synth.tile_problem without the per-trajectory arrays (those are tiled on the device)."""
    from trajoptkp_amd import synth
    empty = np.zeros((p["batch"], 0))
    return synth.tile_problem(dict(p, r=empty, r_x=empty, r_u=empty, u_nom=empty), reps)


# ---- the bytes of every device buffer ---------------------------------------------------------------------------------------------
def entries_per_unique_set(c):
    return sum(len(l) for u in range(UNIQ) for l in kp_lists(c, u))


def buffers(c):
    """name -> dict(bytes, and for the per-trajectory buffers: inner, unit, elem -- [batch][inner][unit elements of `elem` bytes]).
    kpilqr_api.cpp: size_buffers (:185-210), the payload slabs (fd_layout :1166-1179, fdkp_layout :1257-1262; an eighth of slack +
    4 KB, :70), the column and slope stores (:237-259; a quarter + 4 KB, :69), the entry tables (:273-283), the staging area of
    U_alpha (:2309); RecLayout::stride (common.h:29-37)."""
    B, T, dof, m, nr, na = c["batch"], c["T"], c["dof"], c["m"], c["nr"], c["n_alpha"]
    n = 2 * dof
    fused = is_fused(c)
    stride = S.rec_stride(n, m)
    out = {}

    def per(name, inner, unit, elem=8):
        out[name] = dict(bytes=B * inner * unit * elem, inner=inner, unit=unit, elem=elem)

    if not fused:
        per("records", T, stride)
        per("segent", dof * T, 1, 4)
    per("K", T, n * m)
    per("k", T, m)
    per("r", T + 1, nr)
    per("r_x", T + 1, nr * n)
    per("r_u", T + 1, nr * m)
    per("u_nom", T, m)
    per("U_alpha", na * T, m)                   # the staging area: [batch][n_alpha][T][m]
    per("segmap", dof * T, 1, 8)
    out["per_trajectory_scalars"] = dict(bytes=B * (8 * 3 + 8 * na + 4 * 4))       # lambda, delta_J, traj_cost, cost_pred, status, attempts, gate, traj_list
    E = entries_per_unique_set(c) * c["reps"]
    out["kp_lists"] = dict(bytes=(B * dof + 1) * 4 + E * 4 + E + 64 * 4)
    if c["payload"] == "kp_ordered":
        need = E * (6 * n + 2) * 8
        out["payload"] = dict(bytes=need + need // 8 + 4096, entries=E, entry_bytes=(6 * n + 2) * 8)
    else:
        # jobs: a uniform set has every column at every key-point (2 dof + m), per-DoF lists the columns of the listed DoFs
        if c["uniform"]:
            J = (E // dof) * (2 * dof + m)
        else:
            J = sum(len(l) * (3 if d < m else 2) for u in range(UNIQ) for d, l in enumerate(kp_lists(c, u))) * c["reps"]
        al16 = lambda x: (x + 15) & ~15
        need = 2 * al16(J * n * 8) + al16(E * n * 8) + 4 * al16(J * 4) + al16(J)       # (xnom: at most one row per entry)
        out["payload"] = dict(bytes=need + need // 8 + 4096, entries=J, entry_bytes=2 * n * 8)
    if fused or c["payload"] == "kp_ordered":   # the column store and the entry tables of a by-entry payload / a fused context
        need = E * 3 * n * 8
        out["kp_columns"] = dict(bytes=need + need // 4 + 4096)
        out["kp_entry"] = dict(bytes=B * dof * T * 4 + E * 4 + 4)
    if fused and not c["uniform"]:
        need = E * 6 * n * 8
        out["kp_slopes"] = dict(bytes=need + need // 4 + 4096)
    return out


def total_bytes(c):
    return sum(b["bytes"] for b in buffers(c).values())


def largest_input(c):
    """(name, elements) of the buffer the issue's first threshold is about: the step records of a materialising family, the per-step
    r_x or the payload of a fused one."""
    bufs = buffers(c)
    if not is_fused(c):
        return "records", bufs["records"]["bytes"] // 8
    cand = {"payload": bufs["payload"]["bytes"] // 8}
    if c["rx"] == "step":
        cand["r_x"] = bufs["r_x"]["bytes"] // 8
    name = max(cand, key=cand.get)
    return name, cand[name]


def crossed(nbytes, elem=8):
    """The thresholds a buffer of nbytes is past."""
    return tuple(k for k, v in THRESHOLDS.items() if (nbytes // elem if k == "elems31" else nbytes) > v)


def held_buffers(c):
    """The per-trajectory buffers past a threshold whose CONTENT differs from one (seed, step) to the next, so that a truncated access
    changes a result: not r_x / r_u of a constant-Jacobian case (one matrix everywhere / zeros), not the maps of a uniform set."""
    out = {}
    for name, b in buffers(c).items():
        if "inner" not in b or not crossed(b["bytes"], b["elem"]):
            continue
        if c["rx"] == "const" and name in ("r_x", "r_u"):
            continue
        if name in ("segmap", "segent"):
            continue
        out[name] = b
    return out


# ---- where a truncated offset lands ----------------------------------------------------------------------------------------------
TRUNCATIONS = (("byte offset mod 2^32", "bytes", 2 ** 32), ("byte offset mod 2^31", "bytes", 2 ** 31),
               ("element offset mod 2^31", "elems", 2 ** 31), ("element offset mod 2^32", "elems", 2 ** 32))


def aliased(c, name, b=None, checked=None):
    """For every trajectory the GPU test holds to the oracle (the last UNIQ) and every unit (step) of buffer `name`: the unit a
    truncated offset of its first and of its last element falls into.  Returns (wrapped, same): how many (truncation, trajectory,
    unit) offsets change under a truncation, and how many of those land in a unit of the same seed at the same step -- where the
    data are the true ones and the truncation would go unnoticed."""
    b = buffers(c)[name] if b is None else b
    B, inner, unit, elem = c["batch"], b["inner"], b["unit"], b["elem"]
    trajs = np.arange(B - UNIQ, B, dtype=np.int64) if checked is None else np.asarray(checked, np.int64)
    i = np.arange(inner, dtype=np.int64)
    first = ((trajs[:, None] * inner + i[None, :]) * unit)             # element offsets [traj][unit]
    wrapped = same = 0
    for _, kind, mod in TRUNCATIONS:
        for off in (first, first + unit - 1):
            loc = (off * elem % mod) // elem if kind == "bytes" else off % mod
            moved = loc != off
            bb, ii = np.divmod(loc // unit, inner)
            hit = moved & (bb % UNIQ == (trajs % UNIQ)[:, None]) & (ii == i[None, :])
            wrapped += int(moved.sum()); same += int(hit.sum())
    return wrapped, same


def inputs_differ(c, p, name, b=None):
    """The host-array side of aliased(): for input buffer `name` of problem p (r, r_x, r_u, u_nom), the data at every location a
    truncated offset of a checked unit lands in differ from the true unit's."""
    b = buffers(c)[name] if b is None else b
    B, inner, unit, elem = c["batch"], b["inner"], b["unit"], b["elem"]
    host = p[name].reshape(UNIQ, inner, unit)
    trajs = np.arange(B - UNIQ, B, dtype=np.int64)
    i = np.arange(inner, dtype=np.int64)
    first = (trajs[:, None] * inner + i[None, :]) * unit
    bad = 0
    for _, kind, mod in TRUNCATIONS:
        loc = (first * elem % mod) // elem if kind == "bytes" else first % mod
        moved = loc != first
        bb, ii = np.divmod(loc // unit, inner)
        true = host[(trajs % UNIQ)[:, None], i[None, :]]
        there = host[bb % UNIQ, ii]
        bad += int((moved & np.all(true == there, axis=-1)).sum())
    return bad


# ---- the largest horizon a sweep form addresses inside one trajectory -------------------------------------------------------------
# form -> (what limits it, the largest T as a function of (dof, m, nr), citations [(file, line, regex the line must match)], guard)
BIGOFF = S.BIGOFF


def _fused_guard_T(dof, m, nr):
    return (BIGOFF - 1) // (dof * (12 * dof + 2) * 8)                    # T * dof * (6 n + 2) * 8 < BIGOFF


def _fused_desc_T(dof, m, nr):
    n = 2 * dof
    return min((2 ** 31 - 1) // (m * n * 8), (2 ** 31 - 1) // (nr * n * 8) - 1, (2 ** 31 - 1) // (nr * m * 8) - 1)


def _fsc_records_T(dof, m, nr):
    return S.FSC_REC_BYTES_MAX // (S.rec_stride(2 * dof, m) * 8)


def _fsc_gains_T(dof, m, nr):
    return (2 ** 31 - 1) // (m * 2 * dof * 8)


HORIZON_LIMITS = {
    "fused_payload": dict(
        what="the key-point ordered payload of one trajectory under one descriptor, entry offsets below BIGOFF: T dof (6n + 2) 8 < 2^30",
        max_T=_fused_guard_T, guard="fused_supported: a longer horizon is not fused (kpilqr_create picks the materialising family)",
        cites=[("fused_mfma.hip", 44, r"^#define BIGOFF 0x40000000$"),
               ("fused_mfma.hip", 2572, r"\(long long\)T \* dof \* \(6 \* n \+ 2\) \* 8 < \(long long\)BIGOFF")]),
    "fused_forward_descriptors": dict(
        what="K, k, u_nom, r_x, r_u, r of one trajectory under one descriptor each, sized as int: T m n 8, (T + 1) nr n 8 < 2^31",
        max_T=_fused_desc_T, guard="inside fused_payload's bound for every one-tile shape (asserted)",
        cites=[("fused_mfma.hip", 1910, r"kp_rsrc\(Kin \+ \(size_t\)b \* T \* m \* n, T \* m \* n \* 8\)"),
               ("fused_mfma.hip", 1911, r"rRx = kp_rsrc\(rxb, \(T \+ 1\) \* nr \* n \* 8\)"),
               ("fused_mfma.hip", 2249, r"kp_rsrc\(Kin \+ \(size_t\)b \* T \* m \* n, T \* m \* n \* 8\)")]),
    "tiled_fsc_records": dict(
        what="the state / cost waves: one trajectory's records under one descriptor, the step in a 32-bit scalar offset: T stride 8 <= 0x7fffff00",
        max_T=_fsc_records_T, guard="forward_tiled_sc_selected: a longer horizon runs the general tiled forward sweep (size_t step bases)",
        cites=[("tiled_mfma.hip", 27, r"^#define KP_FSC_REC_BYTES_MAX 0x7fffff00u$"),
               ("tiled_mfma.hip", 1524, r"rRec = kp_rsrc\(rec \+ \(size_t\)b \* T \* L\.stride, \(int\)\(\(size_t\)T \* L\.stride \* 8 < KP_FSC_REC_BYTES_MAX"),
               ("tiled_mfma.hip", 1530, r"const int so = \(t < T \? t : T - 1\) \* recB;"),
               ("tiled_mfma.hip", 1689, r"rRec = kp_rsrc\(rec \+ \(size_t\)b \* T \* L\.stride, \(int\)\(\(size_t\)T \* L\.stride \* 8 < KP_FSC_REC_BYTES_MAX"),
               ("tiled_mfma.hip", 1821, r"if \(\(size_t\)c->d\.T \* c->L\.stride \* 8 > KP_FSC_REC_BYTES_MAX\) return false;")]),
    "tiled_fsc_gains": dict(
        what="the state / cost waves: K, k, u_nom of one trajectory under one descriptor each, sized as int: T m n 8 < 2^31",
        max_T=_fsc_gains_T, guard="unreachable: a record is larger than K's step (stride > m n), so tiled_fsc_records ends the form first (asserted)",
        cites=[("tiled_mfma.hip", 1525, r"rKt = kp_rsrc\(Kin \+ \(size_t\)b \* T \* m \* n, T \* m \* n \* 8\);"),
               ("tiled_mfma.hip", 1526, r"rkt = kp_rsrc\(kin \+ \(size_t\)b \* T \* m, T \* m \* 8\);"),
               ("tiled_mfma.hip", 1527, r"rut = kp_rsrc\(u_nom \+ \(size_t\)b \* T \* m, T \* m \* 8\);")]),
}
# Every other sweep rebuilds its descriptors per step on a size_t base ((size_t)b * T + t) * ..., e.g. riccati_mfma.hip:157-158,
# forward_mfma.hip:72-75, tiled_mfma.hip:190, 531-532, tiled_wide.hip:168, 373-374, generic.hip:190-197, 323-326): no in-trajectory limit
# below 2^31 ELEMENTS of one trajectory's records, which at the largest shape (n = 62, 65 920 B per step) is a horizon of 260 000
# steps and 17 GB for B = 1 -- inside CAP, and not pinned by any test ("Offsets beyond 32 bits").


def cited_lines(csrc=CSRC):
    """[(form, file, line, regex, the text of that line)]"""
    out, cache = [], {}
    for form, spec in HORIZON_LIMITS.items():
        for name, line, pat in spec["cites"]:
            if name not in cache:
                cache[name] = open(os.path.join(csrc, name)).read().split("\n")
            out.append((form, name, line, pat, cache[name][line - 1]))
    return out


def stale_citations(csrc=CSRC):
    return [(form, f"{name}:{line}", text.strip()) for form, name, line, pat, text in cited_lines(csrc) if not re.search(pat, text)]


# ---- the in-trajectory limit of the state / cost waves, at the widest two-tile shape -------------------------------------------------
FSC_SHAPE = dict(dof=15, m=8, nr=4)
FSC_T_INSIDE = _fsc_records_T(**FSC_SHAPE)      # 125 203: the last horizon the form addresses
FSC_T_BEYOND = FSC_T_INSIDE + 1                 # 125 204: the first one it does not


# ---- the printed table ------------------------------------------------------------------------------------------------------------
def table():
    lines = [f"{'case':18s} {'(n, m, nr)':12s} {'T':>4s} {'B':>6s} {'total GB':>9s}  largest input (elements)      K bytes        buffers past a threshold"]
    for c in CASES:
        bufs = buffers(c)
        name, el = largest_input(c)
        past = ", ".join(f"{k} {b['bytes'] / 1e9:.2f} GB [{'/'.join(crossed(b['bytes'], b.get('elem', 8)))}]" for k, b in bufs.items()
                         if crossed(b["bytes"], b.get("elem", 8)))
        lines.append(f"{c['name']:18s} {str((2 * c['dof'], c['m'], c['nr'])):12s} {c['T']:4d} {c['batch']:6d} {total_bytes(c) / 1e9:9.2f}  "
                     f"{name:8s} {el:13d} {'>' if el > 2 ** 31 else '<'} 2^31  {bufs['K']['bytes']:11d} {'>' if bufs['K']['bytes'] > 2 ** 32 else '<'} 2^32  {past}")
    return "\n".join(lines)
