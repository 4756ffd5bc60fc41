"""Cases of key-point placement on the device for a listed subset of the batch (tests/test_gpu_keypoints_partial.py on the GPU,
tests/test_keypoints_partial_inputs.py on the CPU): states from the generator of tests/test_gpu_parity.py, lists from the oracle's
kp_* functions.  Every case is (states X0 the whole batch is placed from, states X1 of which the LISTED trajectories' rows go up
through kpilqr_upload_states_partial, the placement arguments of both calls); what the device must hold afterwards is the oracle's
lists of X1 for a listed trajectory and of X0 for everybody else.

No GPU code runs at import."""
import functools

import numpy as np

from oracle import oracle as orc
from test_gpu_parity import _kp_states
from trajoptkp_amd import synth
from trajoptkp_amd.engine import rows_to_dof_csr

METHODS = ("set_interval", "adaptive_jerk", "adaptive_accel", "velocity_change")
# (dof, T, batch): T below the jerk stencil (2, 3), a chunk of exactly 64 steps, one step into the next chunk, two chunks and a tail;
# dof 7 and 31 for the staging loop's row length
SHAPES = [(3, 2, 5), (3, 3, 5), (3, 64, 5), (3, 65, 5), (3, 130, 6), (7, 65, 4), (31, 65, 3)]
SUBSETS = ("first", "last", "pair", "all")
SEED, MIN_N, MAX_N, DT = 11, 2, 20, 0.01
# set_interval reads no states: the listed trajectories are placed with another interval, so that their lists change (from T = 4 on)
MIN_N_LISTED_INTERVAL = 3
MANY = (7, 20, 48)               # more than one block of k_kp_fill (256 lists): 41 scattered trajectories of 48, 287 lists
CARRY = dict(task="panda_reaching", T=65, batch=4, traj=[1, 2], method="velocity_change")


def subset(name, B):
    """The first trajectory alone, the last alone, a scattered pair, everybody."""
    return {"first": [0], "last": [B - 1], "pair": [0, B - 2] if B > 3 else [0, B - 1], "all": list(range(B))}[name]


def many_subset():
    B = MANY[2]
    return [b for b in range(B) if b % 7 != 3]          # 41 of 48: runs of six with single gaps, both ends listed


def thresholds(rng, method, dof):
    """As tests/test_gpu_parity.py::test_device_keypoint_generation_matches_oracle draws them."""
    if method == "adaptive_jerk":
        return rng.uniform(50.0, 4000.0, dof)
    if method == "adaptive_accel":
        return rng.uniform(0.005, 0.2, dof)
    return rng.uniform(0.5, 20.0, dof)


def states(rng, dof, T, B):
    return np.stack([_kp_states(rng, dof, T) if T > 8 else rng.standard_normal((T, 2 * dof)) for _ in range(B)])


def oracle_rows(method, dof, T, min_N, max_N, thr, X):
    """The oracle's placement for every trajectory of X [B][T][2 dof], as the reference's rows (offs [T+1], cols)."""
    out = []
    for Xb in X:
        if method == "set_interval":
            out.append(orc.kp_set_interval(dof, T, min_N))
        elif method == "adaptive_jerk":
            out.append(orc.kp_adaptive_jerk(dof, T, min_N, max_N, thr, DT, Xb))
        elif method == "adaptive_accel":
            out.append(orc.kp_adaptive_accel(dof, T, min_N, max_N, thr, Xb))
        else:
            out.append(orc.kp_velocity_change(dof, T, min_N, max_N, thr, Xb))
    return out


def dof_lists(rows, dof, T):
    """rows of one trajectory -> its per-DoF lists (the oracle may name a DoF twice at the last step: a list holds the step once)."""
    o, t = rows_to_dof_csr([rows], dof, T)
    return [np.unique(t[o[i]:o[i + 1]]) for i in range(dof)]


def csr(lists_per_traj):
    """[trajectory][dof] lists -> (offsets from 0, times): the per-DoF CSR of include/kpilqr.h."""
    flat = [np.asarray(l, np.int32) for lists in lists_per_traj for l in lists]
    offs = np.concatenate([[0], np.cumsum([len(l) for l in flat])]).astype(np.int32)
    return offs, (np.concatenate(flat) if flat else np.zeros(0, np.int32)).astype(np.int32)


def merged(lists0, lists1, traj):
    return [lists1[b] if b in traj else lists0[b] for b in range(len(lists0))]


def _case(method, dof, T, B, seed=SEED, thr=None):
    rng = np.random.default_rng(seed)
    X0, X1 = states(rng, dof, T, B), states(rng, dof, T, B)
    thr = thresholds(rng, method, dof) if thr is None else thr
    min1 = MIN_N_LISTED_INTERVAL if method == "set_interval" else MIN_N
    lists0 = [dof_lists(r, dof, T) for r in oracle_rows(method, dof, T, MIN_N, MAX_N, thr, X0)]
    lists1 = [dof_lists(r, dof, T) for r in oracle_rows(method, dof, T, min1, MAX_N, thr, X1)]
    th = None if method == "set_interval" else thr
    return dict(method=method, dof=dof, T=T, batch=B, X0=X0, X1=X1, lists0=lists0, lists1=lists1,
                args0=(method, MIN_N, MAX_N, th, DT), args1=(method, min1, MAX_N, th, DT))


@functools.lru_cache(maxsize=None)
def list_case(method, shape):
    return _case(method, *shape)


@functools.lru_cache(maxsize=None)
def many_case():
    return _case("velocity_change", *MANY)


@functools.lru_cache(maxsize=None)
def carry_case():
    """The payload-carry case: Panda reaching on a fused context, the middle pair re-placed, trajectory 3 kept BEHIND them."""
    cfg = synth._task_cfg(CARRY["task"])[1]
    c = _case(CARRY["method"], cfg["dof"], CARRY["T"], CARRY["batch"])
    c.update(task=CARRY["task"], traj=list(CARRY["traj"]))
    return c


def entries(lists):
    """Entries of one trajectory."""
    return int(sum(len(l) for l in lists))


def first_entry(lists_per_traj, b):
    return int(sum(entries(l) for l in lists_per_traj[:b]))


def rows_of(lists, dof, T):
    """Per-DoF lists of one trajectory -> the rows synth.make_ragged_problem takes."""
    return synth.rows_from_dof_lists(dof, T, [list(map(int, l)) for l in lists])
