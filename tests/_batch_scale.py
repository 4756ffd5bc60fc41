"""Problems and references of tests/test_gpu_batch_scale.py (checked on the CPU by tests/test_batch_scale_inputs.py): batches whose
list and trajectory counts outgrow one workgroup of the kernels AROUND the sweeps -- key-point placement, entry tables, segment maps,
the uniform flag, row / gain movers, subset lists -- with every trajectory DISTINCT.  No synth.tile_problem here: every trajectory has
its own seed (synth.seed_for(config_id, b)), so a kernel that reads trajectory b +- k, b mod k, or swaps two blocks cannot pass.
No GPU is needed to import or to run anything in this file; N_SIMD is the MI355X's 1024 for the CPU checks, the GPU tests read the
device's (_shape_run._n_simd()) and pass it in.

What the builders assert themselves (distinct()): the per-trajectory inputs differ pairwise, and the oracle's cost_pred[:, 0] and
K[0] take one value per trajectory (over the trajectories whose oracle status is 0), so two aliased rows cannot cancel.

Oracle statuses found (status != 0 / trajectories; lam = 0.1, the config ids below), n_simd = 1024:
  section 1b  (2, 1025) and (7, 293), both methods:                                   0 / 1025, 0 / 293
  section 1c  Panda T = 24, B = 1025, odd trajectory at 0 / 512 / 1024, and without:  0 / 1025 each;  T = 300, B = 3:  0 / 3
  section 2   every case of bound_cases(1024):                                        0 / batch each
  section 3   base problem, the three regenerated problems:                           0 / 1025 each
so the 99 % figure holds with nothing to spare needed, and no trajectory's gains go uncompared.

Ragged lists.  "Neighbouring lists differ in length" is asserted (tests/test_batch_scale_inputs.py) at >= 90 % of adjacent pairs for
every set of per-DoF lists this file chooses freely: sections 1b and 3, and the adaptive placements of 1a at T >= 64.  It cannot
hold, and is not asked, where the lists are fixed by the case: set_interval (one list for all), the uniform shapes of
_shapes.batch_cases (their dispatch is asserted as ":uni"), section 1c (set_interval but one key-point), and T = 5, where a list has
2 .. 5 entries and two neighbours agree by chance far more often than one time in ten -- there the lists must still take more
than one length."""
import functools

import numpy as np

import _shape_run as R
import _shapes as S
from _sequences import _kp_states
from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import synth
from trajoptkp_amd.engine import rows_to_dof_csr

N_SIMD = 1024
RTOL = 1e-9                     # the suite's bar against the oracle (tests/_shape_run.py, TIGHT in tests/test_gpu_configs.py)
ALPHAS = orc.alphas(6)
JOBS = ("job_b", "job_t", "job_col", "job_mode", "job_nom", "xplus", "xminus")
PER_TRAJ = ("r", "r_x", "r_u", "u_nom")


# ---- what every problem is held to -------------------------------------------------------------------------------------------------
def references(p, n_alpha=6, lam=None):
    """The oracle of every trajectory.  lam: [batch] or None (the problem's)."""
    return [pipeline.run_trajectory(p, b, lam=None if lam is None else float(lam[b]), n_alpha=n_alpha, want_U=True) for b in range(p["batch"])]


def references_on_columns(p, rows, cols, lam, n_alpha=6):
    """The oracle of every trajectory of p on other data than p's own: per-trajectory inputs `rows` (r, r_x, r_u, u_nom, each [batch]...)
    and key-point columns cols [entries][3][n] in the order of p's lists (kind 0 / 1 / 2: column d of A, d + dof of A, d of B).
    lam: [batch].  Interpolation, cost derivatives, backward and forward sweep; the lists are turned into a CSR once."""
    dof, n, m, nr, T = p["dof"], p["n"], p["m"], p["nr"], p["T"]
    offs, times = rows_to_dof_csr(p["kp_rows"], dof, T)
    al = orc.alphas(n_alpha)
    out = []
    for b in range(p["batch"]):
        A = np.zeros((T, n, n)); B = np.zeros((T, m, n))
        for d in range(dof):
            e0, e1 = int(offs[b * dof + d]), int(offs[b * dof + d + 1])
            ts = times[e0:e1]
            A[ts, d, :] = cols[e0:e1, 0]
            A[ts, d + dof, :] = cols[e0:e1, 1]
            if d < m:
                B[ts, d, :] = cols[e0:e1, 2]
        o, c = p["kp_rows"][b]
        orc.interpolate(dof, m, T, o, c, A, B)
        l_x, l_xx, l_u, l_uu = orc.cost_derivs(n, m, nr, T, rows["r"][b], rows["r_x"][b], rows["r_u"][b], p["w_run"], p["w_term"])
        st, K, k, dJ = orc.backward(n, m, T, A, B, l_x, l_xx, l_u, l_uu, float(lam[b]), 100)
        res = dict(status=st, K=K, k=k, delta_J=dJ)
        if st == 0:
            res["cost_pred"] = orc.forward_linear(n, m, T, al, A, B, K, k, l_x, l_xx, l_u, l_uu, rows["u_nom"][b], p["ctrl_lim"])
        out.append(res)
    return out


def distinct(p, refs):
    """Asserts B pairwise distinct trajectories: inputs, and the oracle's cost_pred[:, 0] and K[0].  Returns the count of status != 0."""
    B = p["batch"]
    assert len(np.unique(p["r"].reshape(B, -1), axis=0)) == B and len(np.unique(p["u_nom"].reshape(B, -1), axis=0)) == B
    ok = [o for o in refs if o["status"] == 0]
    assert len(np.unique([o["cost_pred"][0] for o in ok])) == len(ok), "cost_pred[:, 0] takes fewer values than trajectories"
    assert len(np.unique(np.stack([o["K"][0].reshape(-1) for o in ok]), axis=0)) == len(ok), "K[0] takes fewer values than trajectories"
    return B - len(ok)


def list_lengths(rows, dof, T):
    offs, _ = rows_to_dof_csr(rows, dof, T)
    return np.diff(offs)


def ragged_fraction(lengths):
    """The fraction of adjacent lists (in CSR order, across trajectories too) whose lengths differ."""
    return float(np.mean(np.diff(lengths) != 0))


def hold(got, refs, rows, tag, keys=("K", "k", "delta_J", "cost")):
    """Trajectories `rows` of a GPU result (dict of [batch]... arrays: status, K, k, delta_J, cost, U) against their oracles at RTOL.
    Where the oracle's status is not 0 the GPU's must equal it and nothing else of that trajectory is compared."""
    for b in rows:
        o = refs[b]
        assert got["status"][b] == o["status"], (tag, b, got["status"][b], o["status"])
        if o["status"] != 0:
            continue
        errs = {}
        for key in keys:
            if key == "delta_J":
                errs[key] = abs(got[key][b] - o[key]) / max(abs(o[key]), 1e-300)
            else:
                errs[key] = R._rel(got[key][b], o[{"cost": "cost_pred", "U": "U_alpha"}.get(key, key)])
        assert max(errs.values()) <= RTOL, (tag, b, errs)


# ---- section 1a: device key-point placement at list counts around 1024 and 2048 -------------------------------------------------------
# (dof, B); (64, 17) -- 1088 lists, dof at the wave's width -- is dropped: kpilqr_create refuses the generic context (the backward
# sweep's LDS bound, _shapes.generic_max_dof: 46 DoFs at m = 7 and never 64), as tests/test_batch_scale_inputs.py asserts
KP_SHAPES = ((2, 511), (2, 512), (2, 513), (2, 1025), (7, 147), (7, 293), (31, 34), (33, 32))
KP_LISTS = (1022, 1024, 1026, 2050, 1029, 2051, 1054, 1056)
KP_DROPPED = ((64, 17),)
KP_HORIZONS = (5, 64, 65, 130)          # below, at and above one 64-step mask chunk, and three chunks
KP_METHODS = ("set_interval", "adaptive_jerk", "adaptive_accel", "velocity_change")
KP_DT = 0.01


def kp_context(dof):
    """The context of a placement case, as tests/test_gpu_parity.py::test_device_keypoint_generation_matches_oracle builds it:
    keywords of Engine (batch and T aside)."""
    return dict(dof=dof, m=min(dof, 7), nr=3, generic=(2 * dof + 2 > 64))


@functools.lru_cache(maxsize=8)
def kp_states(dof, B, T):
    """[B][T][2 dof]: _kp_states, one random stream per trajectory"""
    return np.stack([_kp_states(np.random.default_rng([dof, T, b]), dof, T) for b in range(B)])


KP_PROBE, KP_PROBE_RAGGED = 48, 0.94
# per-DoF thresholds, log-uniform over the bulk of each profile on _kp_states (velocity noise of about 1.4 per step at dt = 0.01:
# jerks of some 1e4, velocity steps of about 2, |v| of up to 10 per step summed between key-points)
KP_THRESHOLDS = {"adaptive_jerk": (5e3, 2e5), "adaptive_accel": (0.3, 6.0), "velocity_change": (3.0, 80.0)}


@functools.lru_cache(maxsize=None)
def kp_params(method, dof, T):
    """(min_N, max_N, thresholds [dof] or None), drawn from default_rng([dof, T, method, k]).  For the adaptive methods at T >= 64 the
    draw is the first k whose ORACLE placement on a probe of 48 trajectories is ragged enough (neighbouring lists of different length
    in 94 % of the pairs; the real shapes are then held to 90 % by tests/test_batch_scale_inputs.py), at T = 5 the first whose
    lists take more than one length: the choice looks at the reference's lists alone."""
    mi = KP_METHODS.index(method)
    if method == "set_interval":
        return int(np.random.default_rng([dof, T, mi]).integers(1, 5)), 1, None
    lo, hi = KP_THRESHOLDS[method]
    for k in range(200):
        rng = np.random.default_rng([dof, T, mi, k])
        min_N, max_N = int(rng.integers(1, 4)), int(rng.integers(8, 40))
        thr = np.exp(rng.uniform(np.log(lo), np.log(hi), dof))
        lengths = list_lengths(kp_rows(method, dof, T, kp_states(dof, KP_PROBE, T), min_N, max_N, thr), dof, T)
        if ragged_fraction(lengths) >= KP_PROBE_RAGGED or (T < 64 and len(np.unique(lengths)) > 1):
            return min_N, max_N, thr
    raise AssertionError(("no ragged placement found", method, dof, T))


def kp_rows(method, dof, T, X, min_N, max_N, thr):
    """the oracle's rows (CSR over time) of every trajectory of X"""
    if method == "set_interval":
        return [orc.kp_set_interval(dof, T, min_N)] * len(X)
    if method == "adaptive_jerk":
        return [orc.kp_adaptive_jerk(dof, T, min_N, max_N, thr, KP_DT, x) for x in X]
    if method == "adaptive_accel":
        return [orc.kp_adaptive_accel(dof, T, min_N, max_N, thr, x) for x in X]
    return [orc.kp_velocity_change(dof, T, min_N, max_N, thr, x) for x in X]


def kp_reference(method, dof, B, T):
    """(offsets [B dof + 1], times) of the oracle's placement, through rows_to_dof_csr"""
    min_N, max_N, thr = kp_params(method, dof, T)
    return rows_to_dof_csr(kp_rows(method, dof, T, kp_states(dof, B, T), min_N, max_N, thr), dof, T)


# ---- section 1b: lists placed by the device drive a whole iteration -----------------------------------------------------------------
FEED_SHAPES = {(2, 1025): "acrobot", (7, 293): "panda_reaching"}
FEED_T = 24
FEED_METHODS = {"velocity_change": (1, 12), "adaptive_jerk": (1, 12)}          # method -> (min_N, max_N)


@functools.lru_cache(maxsize=None)
def feed_thresholds(method, dof):
    """per-DoF thresholds: the first draw whose oracle placement on the probe is ragged enough, as kp_params chooses"""
    lo, hi = KP_THRESHOLDS[method]
    min_N, max_N = FEED_METHODS[method]
    X = kp_states(dof, KP_PROBE, FEED_T)
    for k in range(200):
        thr = np.exp(np.random.default_rng([77, dof, KP_METHODS.index(method), k]).uniform(np.log(lo), np.log(hi), dof))
        if ragged_fraction(list_lengths(kp_rows(method, dof, FEED_T, X, min_N, max_N, thr), dof, FEED_T)) >= KP_PROBE_RAGGED:
            return thr
    raise AssertionError(("no ragged placement found", method, dof))


@functools.lru_cache(maxsize=2)
def feed_problem(dof, B, method):
    """-> (problem, states X, min_N, max_N, thresholds).  FD columns at every step (min_N = 1 job lists), as
    test_device_keypoints_feed_the_pipeline has them, so whatever lists the placement gives find their columns; the problem's
    kp_rows are the ORACLE's placement on X."""
    p = synth.make_problem(task=FEED_SHAPES[(dof, B)], T=FEED_T, batch=B, min_N=1, dense_residuals=True, config_id=21)
    X = kp_states(dof, B, FEED_T)
    min_N, max_N = FEED_METHODS[method]
    thr = feed_thresholds(method, dof)
    p["kp_rows"] = kp_rows(method, dof, FEED_T, X, min_N, max_N, thr)
    p["kp_times"] = None
    return p, X, min_N, max_N, thr


# ---- section 1c: the uniform flag with one odd trajectory ---------------------------------------------------------------------------
UNI_T, UNI_MIN_N, UNI_EXTRA_T = 24, 4, 10       # set_interval(4) on 24 steps: 0 4 8 12 16 20 23; the odd list also has step 10
LONG_T, LONG_B, LONG_GAP, LONG_ODD_GAP = 300, 3, 290, 291


def _by_entry(p):
    """(control columns without a DoF list have no slot in a by-entry payload; none on Panda, kept for the rule)"""
    keep = p["job_col"] < p["n"] + min(p["m"], p["dof"])
    for k in JOBS:
        p[k] = p[k][keep]
    return p


@functools.lru_cache(maxsize=4)
def uniform_problem(B, odd):
    """Panda, T = 24, set_interval(4) lists for every DoF of every trajectory; odd = trajectory whose LAST DoF has one more key-point
    (step 10), or None: nobody (every trajectory's lists are then one list).  The data of a trajectory depend on its own lists and
    index alone, so the two problems differ in trajectory `odd` only."""
    dof = 7
    base = orc.kp_set_interval(dof, UNI_T, UNI_MIN_N)
    times = np.flatnonzero(np.diff(base[0]))
    assert UNI_EXTRA_T not in times
    lists = [list(times)] * (dof - 1) + [sorted(list(times) + [UNI_EXTRA_T])]
    rows = [base] * B
    if odd is not None:
        rows[odd] = synth.rows_from_dof_lists(dof, UNI_T, lists)
    return _by_entry(synth.make_ragged_problem("panda_reaching", UNI_T, rows, config_id=31, dense_residuals=False, one_sided_frac=0.1))


@functools.lru_cache(maxsize=2)
def long_uniform_problem(odd):
    """Panda, T = 300, B = 3, lists of 299 entries: min_N = 1 -- every step -- but step 290.  k_kp_uniform compares two lists of one
    length entry by entry, 256 threads striding over the list, so a difference the stride alone reaches has to sit at an index
    above 256 of two lists of EQUAL length: an every-step list has no room for that (nothing can be added, and a removal changes the
    length, which the kernel tests first), hence the one step left out.  odd: the last DoF of trajectory 2 leaves out step 291
    instead -- its list differs from its neighbours' at index 290 and nowhere else.  odd = False: nobody."""
    dof, T = 7, LONG_T
    base = [t for t in range(T) if t != LONG_GAP]
    other = [t for t in range(T) if t != LONG_ODD_GAP]
    assert len(base) == len(other) > 256 and [i for i in range(len(base)) if base[i] != other[i]] == [LONG_GAP]
    rows = [synth.rows_from_dof_lists(dof, T, [base] * dof)] * LONG_B
    if odd:
        rows[2] = synth.rows_from_dof_lists(dof, T, [base] * (dof - 1) + [other])
    return _by_entry(synth.make_ragged_problem("panda_reaching", T, rows, config_id=32, dense_residuals=False, one_sided_frac=0.1))


# ---- section 2: distinct trajectories on both sides of every batch bound -------------------------------------------------------------
BOUND_T = 12
BOUND_CONFIG = 5


def bound_cases(n_simd):
    """The shapes of _shapes.batch_cases at T = 12 -- the fused ones with a constant and with per-step r_x --, the consumer / helper
    pair of the fused Panda sweeps at n_simd / 2 and one more (the one-wave forms), and one fused case with eight alphas above n_simd
    (the paired scoring of the one-wave forward sweep at batch scale)."""
    out = []
    for c in S.batch_cases(n_simd):
        c = dict(c, T=BOUND_T)
        out.append(c)
        if c["flags"] & S.FLAG_FUSED:
            out.append(dict(c, rx_const=False))
    for b in (n_simd // 2, n_simd // 2 + 1):
        for rxc in (True, False):
            out.append(S._case(7, 7, 9, S.FLAG_FUSED, T=BOUND_T, batch=b, rx_const=rxc, why="pair"))
    out.append(S._case(7, 7, 9, S.FLAG_FUSED, T=BOUND_T, batch=n_simd + 1, n_alpha=8, rx_const=True, why="alpha8"))
    return out


def bound_problem(c):
    """B distinct seeds (make_problem seeds every trajectory by its index)"""
    return R._problem(c, config_id=BOUND_CONFIG)


# ---- section 3: listed calls with long, scattered lists ------------------------------------------------------------------------------
LISTED_T = 24
LISTED_CONFIG = (41, 42)          # the data of the base problem | of regenerated trajectories


def listed_lists(B):
    """every third trajectory | a random strictly increasing half | all but one (an interior one) | the streamed ring's fourth: every
    third from 2.  Every list holds trajectory 0 and trajectory B - 1."""
    rng = np.random.default_rng(B)
    half = np.sort(np.concatenate([[0, B - 1], 1 + rng.choice(B - 2, size=B // 2 - 2, replace=False)]))
    ends = {0, B - 1}
    return {"third": sorted(ends | set(range(0, B, 3))), "half": [int(b) for b in half], "all_but_one": [b for b in range(B) if b != B // 3],
            "third_from_2": sorted(ends | set(range(2, B, 3)))}


def ragged_rows(seed, b, dof=7, T=LISTED_T):
    """Per-DoF lists of one trajectory: ends always, the rest random; the lengths walk so that no DoF has its predecessor's (the first
    DoF of trajectory b follows the last of b - 1: lengths are drawn from two disjoint sets by the parity of b * dof + i)."""
    rng = np.random.default_rng([seed, b])
    lists = []
    for i in range(dof):
        odd = (b * dof + i) % 2
        length = int(rng.choice(np.arange(2 + odd, T // 2, 2)))
        mid = rng.choice(np.arange(1, T - 1), size=length - 2, replace=False)
        lists.append(sorted([0, T - 1] + [int(t) for t in mid]))
    return synth.rows_from_dof_lists(dof, T, lists)


@functools.lru_cache(maxsize=8192)
def _piece(b, rows_seed, config_id):
    """One trajectory of a section 3 problem: a function of its index, its lists and its configuration alone"""
    q = synth.make_ragged_problem("panda_reaching", LISTED_T, [ragged_rows(rows_seed, b)], config_id=config_id, one_sided_frac=0.2, first_b=b)
    return _by_entry(q)


def assemble(pieces):
    """One-trajectory problems -> one problem (what make_ragged_problem would have built from all the rows at once)"""
    p = dict(pieces[0])
    nom = np.cumsum([0] + [len(q["xnom"]) for q in pieces])
    p["job_b"] = np.concatenate([np.full(len(q["job_b"]), b, np.int32) for b, q in enumerate(pieces)])
    p["job_nom"] = np.concatenate([q["job_nom"] + np.int32(nom[b]) for b, q in enumerate(pieces)]).astype(np.int32)
    for k in ("job_t", "job_col", "job_mode", "xplus", "xminus", "xnom") + PER_TRAJ:
        p[k] = np.concatenate([q[k] for q in pieces])
    p["kp_rows"] = [q["kp_rows"][0] for q in pieces]
    p["batch"] = len(pieces)
    return p


@functools.lru_cache(maxsize=2)
def listed_base(B):
    return assemble([_piece(b, 1, LISTED_CONFIG[0]) for b in range(B)])


@functools.lru_cache(maxsize=4)
def listed_regenerated(B, name):
    """The base problem with the trajectories of list `name` regenerated: new ragged lists, new FD data, new residuals and nominal
    controls (another configuration); everybody else keeps every byte."""
    who = set(listed_lists(B)[name])
    return assemble([_piece(b, 2, LISTED_CONFIG[1]) if b in who else _piece(b, 1, LISTED_CONFIG[0]) for b in range(B)])


def listed_lambdas(B, which):
    """one lambda per trajectory, so that the resident lambdas say whose they are: 0.05 .. 0.15 before, 0.2 .. 0.3 for listed calls"""
    return (0.05 if which == 0 else 0.2) + 0.1 * (np.arange(B) % 97) / 96.0


def sub(p, who):
    """The trajectories `who` (increasing) of a problem as a problem of their own, in list order (tests/_partial_sweeps.py: sub)."""
    who = np.asarray(who, np.int64)
    q = dict(p)
    sel = np.isin(p["job_b"], who)
    for k in JOBS:
        q[k] = p[k][sel]
    q["job_b"] = np.searchsorted(who, q["job_b"]).astype(np.int32)
    for k in PER_TRAJ:
        q[k] = p[k][who]
    q["kp_rows"] = [p["kp_rows"][b] for b in who]
    q["batch"] = len(who)
    return q
