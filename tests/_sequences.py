"""Model-based sequence tests: ONE long-lived context driven through a random sequence of ABI calls while a Python shadow tracks
what its inputs now are (tests/test_gpu_sequences.py on the GPU, tests/test_sequence_model.py on the CPU, tools/sequence_fuzz.py).

What a context computes depends on the validity flags of Ctx (common.h: PayloadDerived -- kpc_valid, kpc_touched, kps_valid, kpcu_valid,
rec_synced --, ListsDerived -- entry_tables_valid, segent_valid, kpu_valid --, have_rec, kp_known_uniform, kp_canonical, kp_offsets_host_valid, n_pending, rx_const_on,
rx_buf_valid, rx_whole, ru_zero, fd_payload, pipe_dirty).  A flag left set one call too long makes a sweep read yesterday's
linearisation; no kernel is wrong then and no single-shot test reaches the state.  Here every observation is compared with the CPU
oracle on the shadow and with a FRESH context that is given the shadow by the shortest whole-batch route.

The shadow (class Shadow) holds a problem in the shape of synth.make_ragged_problem plus what include/kpilqr.h defines as state: the
resident payload kind, the pending trajectory set, the residual-Jacobian mode, whether r_u was ever written, whether a whole r_x was
given, the shape.  An op is a small dict ({"op": name, ..., "seed": s}): its data are drawn from default_rng(seed) when it is applied,
so a sequence prints as a list that can be cut by hand.  Shadow.apply(op, engine) mutates the shadow and, given an engine, makes
the calls that do the same on the device -- one function per op, so the two cannot drift apart.

No GPU code is imported at module level."""
import contextlib
import copy
import functools
import os

import numpy as np

from oracle import oracle as orc, pipeline
from trajoptkp_amd import synth
from trajoptkp_amd.engine import KpilqrError, rows_to_dof_csr

ERR_ARG, ERR_STATE = -1, -5
RTOL = 1e-9                     # against the oracle: the suite's bar (tests/_shape_run.py)
RTOL_FORMS = 1e-12              # between two forms of the same sweep (raw / column store, per-DoF / union: DESIGN.md section 4.2)
ALPHAS = orc.alphas(6)
BATCH = 4                       # three chunks are 1, 1 and 2 trajectories
HORIZONS = (37, 21)             # two partial 16-step tiles of k_interpolate / k_fd_kp_interpolate; the resize target
EPS = 1e-6                      # a context has one eps
N_OPS, MIN_OBS = 40, 10

# kind -> first task, Engine keywords, environment read by kpilqr_create, (dof, m) of the resize target (nr stays: a resize keeps the
# residual list).  The one-tile fused kinds shrink to an acrobot-sized state; the record kinds change family (one tile <-> tiled); the
# a6 kind stays tiled so that it keeps forming the cost derivatives inside its sweeps.
KINDS = {
    "fused": dict(task="panda_reaching", kw=dict(fused=True), env={}, second=(2, 1)),
    "fused_w1": dict(task="panda_reaching", kw=dict(fused=True), env={"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}, second=(2, 1)),
    "fused_noraw": dict(task="panda_reaching", kw=dict(fused=True), env={"KPILQR_FUSED_RAW": "0"}, second=(2, 1)),
    "fused_union": dict(task="panda_reaching", kw=dict(fused=True, union_keypoints=True), env={}, second=(2, 1)),
    "records_t1": dict(task="panda_reaching", kw=dict(), env={}, second=(10, 7)),
    "records_tiled": dict(task="panda_pushing", kw=dict(), env={}, second=(7, 7)),
    "tiled_a6": dict(task="panda_pushing", kw=dict(fused=True), env={"KPILQR_TILED_A6": "1"}, second=(9, 6)),
}
SEEDS = (42, 43, 44, 45, 46, 47)      # (a window over which every kind shows every op class: tests/test_sequence_model.py)

PAYLOAD_DECK = ["jobs", "jobs_slab", "fd_kp", "cols", "fd_kp", "cols"]       # only a payload laid out by entry survives an update
SUBSETS = {"first": [0], "last": [BATCH - 1], "pair": [1, 2], "all": list(range(BATCH)), "none": []}
STAGE_CALLS = ("fd_difference", "interpolate", "fd_interpolate", "cost_derivs", "fd_interpolate_partial", "cost_derivs_partial", "get_AB",
               "get_union_keypoints", "get_union_columns", "device_ptr_rx", "backward_stats", "get_keypoints", "update_none")
REFUSALS = ("observe_pending", "update_pending", "rx_rows_const", "rx_rows_before_whole", "ru_rows_before_whole", "partial_records_fused",
            "partial_upload_wrong_traj")


def _entries_of(p, traj):
    """CSR entry indices of the listed trajectories of problem p, back to back in traj order."""
    o, _ = rows_to_dof_csr(p["kp_rows"], p["dof"], p["T"])
    dof = p["dof"]
    return np.concatenate([np.arange(o[b * dof], o[(b + 1) * dof]) for b in traj]) if len(traj) else np.zeros(0, np.int64)


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300) if a.size else 0.0


def _kp_states(rng, dof, T):
    """Smooth-ish joint trajectories with a few velocity kinks (what makes velocity_change place per-DoF key-points)."""
    t = np.arange(T)[:, None] * 0.01
    q = np.cumsum(rng.standard_normal((T, dof)) * 0.02, axis=0) + np.sin(t * rng.uniform(1, 9, dof))
    v = np.gradient(q, 0.01, axis=0)
    for _ in range(2 * dof):
        v[int(rng.integers(2, T - 2)):, int(rng.integers(0, dof))] += rng.uniform(-2, 2)
    return np.concatenate([q, v], axis=1)


def _task_of(key):
    return key if isinstance(key, str) else synth.shape_task(*key)


@functools.lru_cache(maxsize=8192)
def _traj_piece(task_key, T, b, cfg_id, offs_bytes, cols_bytes):
    """The FD jobs of ONE trajectory: a function of its index, its lists and the configuration its data were drawn under, so a
    trajectory that keeps its lists (and is not re-uploaded) keeps its records whatever happens to the others."""
    rows = (np.frombuffer(offs_bytes, np.int32), np.frombuffer(cols_bytes, np.int32))
    q = synth.make_ragged_problem(_task_of(task_key), T, [rows], config_id=cfg_id, one_sided_frac=0.3, first_b=b, eps=EPS)
    return {k: q[k] for k in ("job_t", "job_col", "job_mode", "job_nom", "xplus", "xminus", "xnom")}


class Illegal(Exception):
    """An op that the header does not allow in the shadow's state (a bug of the generator, never of the device)."""


class Shadow:
    def __init__(self, kind):
        self.kind, self.K = kind, KINDS[kind]
        self.shape = 0
        self.lam = np.full(BATCH, 0.1)
        self.n_resize = 0
        self._forget()

    # ---- the shape ---------------------------------------------------------------------------------------------------------
    @property
    def task_key(self):
        if self.shape == 0:
            return self.K["task"]
        return self.K["second"] + (synth.TASKS[self.K["task"]]["nr"],)

    @property
    def cfg(self):
        return synth._task_cfg(_task_of(self.task_key))[1]

    @property
    def dims(self):
        c = self.cfg
        return c["dof"], c["m"], HORIZONS[self.shape], c["nr"]

    @property
    def fused(self):
        """The context runs the fused one-tile sweeps at this shape (fused_supported, fused_mfma.hip) and holds no step records."""
        dof, m, _, nr = self.dims
        return bool(self.K["kw"].get("fused")) and 2 * dof + 2 <= 16 and m <= dof and nr <= 16

    @property
    def union(self):
        return self.fused and bool(self.K["kw"].get("union_keypoints"))

    @property
    def a6(self):
        return bool(self.K["kw"].get("fused")) and not self.fused

    def _forget(self):
        """What kpilqr_create leaves and kpilqr_resize forgets: everything uploaded before."""
        dof, m, T, nr = self.dims
        n = 2 * dof
        self.rows, self.pay_cfg, self.payload, self.pending = None, [0] * BATCH, "none", []
        self.r, self.r_x, self.r_u = np.zeros((BATCH, T + 1, nr)), np.zeros((BATCH, T + 1, nr, n)), np.zeros((BATCH, T + 1, nr, m))
        self.u_nom, self.ctrl_lim, self.w_run, self.w_term = np.zeros((BATCH, T, m)), None, None, None
        self.have_r = self.have_nom = False
        self.rx_mode, self.rx_whole, self.ru_written = "step", False, False
        self.sweeps_ran = self.lists_on_host = False          # alphas and lambda resident; kp_traj_first_host
        self.rx_const = np.zeros((nr, n))
        self.rx_const[np.arange(nr), np.arange(nr) % n] = 1.0   # selector rows (Reaching.cpp:43-54), as synth gives a task that has them

    def missing(self):
        """What has to arrive before the header defines the result of a sweep."""
        out = []
        if self.rows is None:
            out.append("kp")
        elif self.payload == "none":
            out.append("payload")
        elif self.pending:
            out.append("pending")
        if not self.have_r:
            out.append("r")
        if self.rx_mode == "step" and not self.rx_whole:
            out.append("rx")
        if self.w_run is None:
            out.append("w")
        if not self.have_nom:
            out.append("nom")
        return out

    # ---- the problem the oracle and a fresh context are given ----------------------------------------------------------------
    def problem(self):
        dof, m, T, nr = self.dims
        n = 2 * dof
        jobs = {k: [] for k in ("job_b", "job_t", "job_col", "job_mode", "job_nom", "xplus", "xminus", "xnom")}
        nom_base = 0
        for b in range(BATCH):
            o, c = self.rows[b]
            q = _traj_piece(self.task_key, T, b, self.pay_cfg[b], np.asarray(o, np.int32).tobytes(), np.asarray(c, np.int32).tobytes())
            jobs["job_b"].append(np.full(len(q["job_t"]), b, np.int32))
            jobs["job_nom"].append(q["job_nom"] + nom_base)
            for k in ("job_t", "job_col", "job_mode", "xplus", "xminus", "xnom"):
                jobs[k].append(q[k])
            nom_base += len(q["xnom"])
        p = {k: np.concatenate(v) for k, v in jobs.items()}
        p.update(task=self.task_key, dof=dof, n=n, m=m, nr=nr, T=T, batch=BATCH, eps=EPS, lam=self.lam.copy(), kp_rows=list(self.rows),
                 r=self.r, r_x=self.r_x, r_u=self.r_u, w_run=self.w_run, w_term=self.w_term, u_nom=self.u_nom, ctrl_lim=self.ctrl_lim,
                 rx_const=self.rx_const)
        return p

    def oracle(self):
        p = self.problem()
        return [pipeline.run_trajectory(p, b, lam=float(self.lam[b]), pd_stride=100, want_U=True) for b in range(BATCH)]

    # ---- data drawn by the ops -----------------------------------------------------------------------------------------------
    def _draw_rows(self, rng, how, b=None):
        dof, _, T, _ = self.dims
        if how == "interval":
            return synth.keypoint_rows_set_interval(dof, T, int(rng.choice([3, 5, 8])))
        if how == "every":
            return synth.rows_from_dof_lists(dof, T, [list(range(T))] * dof)
        if how == "ends":
            return synth.rows_from_dof_lists(dof, T, [[0, T - 1]] * dof)
        return synth.bisect_keypoints(rng, dof, T, 1, rng.uniform(0.2, 1.0, dof))

    def _new_payload_cfg(self, rng, traj):
        for b in traj:
            self.pay_cfg[b] = int(rng.integers(1, 1 << 20))

    def _draw_residuals(self, rng, count, what):
        dof, m, T, nr = self.dims
        r = rng.standard_normal((count, T + 1, nr)) * np.linspace(0.5, 0.05, T + 1)[None, :, None]
        r_x = rng.standard_normal((count, T + 1, nr, 2 * dof)) * 0.3 if "rx" in what else None
        r_u = rng.standard_normal((count, T + 1, nr, m)) * 0.05 if "ru" in what else None
        return r, r_x, r_u

    # ---- legality ------------------------------------------------------------------------------------------------------------
    def illegal(self, op):
        """None, or why the header does not define (or refuses) this op in this state."""
        name = op["op"]
        if name in ("set_keypoints", "generate_keypoints", "lam", "weights", "nominal", "upload_residuals", "rx_const", "resize"):
            return None
        if name == "update_keypoints":
            if self.rows is None:
                return "no key-points yet"
            return "ranges are pending" if self.pending else None
        if name == "upload_payload":
            return "no key-points yet" if self.rows is None else None
        if name == "upload_payload_partial":
            return None if self.pending else "nothing is pending"
        if name == "residuals_partial":
            if "rx" in op["what"] and not (self.rx_mode == "step" and self.rx_whole):
                return "r_x rows of a subset need a whole per-step r_x"
            if "ru" in op["what"] and not self.ru_written:
                return "r_u rows of a subset need a whole r_u"
            return None
        if name == "nominal_partial":
            return None if self.have_nom else "no whole u_nom yet"
        if name == "stage":
            call = op["call"]
            if call == "get_keypoints":
                return "no key-points yet" if self.rows is None else None
            if self.missing():
                return f"state incomplete: {self.missing()}"
            if call in ("fd_interpolate_partial", "cost_derivs_partial") and self.fused:
                return "a fused context refuses the partial record calls"
            if call in ("get_union_keypoints", "get_union_columns") and not self.union:
                return "no union on this context"
            if call == "backward_stats" and not (self.fused and self.sweeps_ran):
                return "fused contexts with a resident lambda only"
            return None
        if name == "refuse":
            which = op["which"]
            ok = {"observe_pending": bool(self.pending), "update_pending": bool(self.pending),
                  "rx_rows_const": self.rx_mode == "const", "rx_rows_before_whole": self.rx_mode == "step" and not self.rx_whole,
                  "ru_rows_before_whole": not self.ru_written, "partial_records_fused": self.fused,
                  "partial_upload_wrong_traj": bool(self.pending)}[which]       # ("`traj` must be exactly the pending set")
            return None if ok else f"the precondition of refusal {which} does not hold"
        if name == "observe":
            streamed = op["how"] == "streamed"
            miss = self.missing()
            if streamed and op.get("payload") and self.rows is not None:
                miss = [x for x in miss if x not in ("payload", "pending")]
            if streamed and "rx" in (op.get("res") or ""):
                miss = [x for x in miss if x not in ("r", "rx")]
            elif streamed and op.get("res"):
                miss = [x for x in miss if x != "r"]
            if miss:
                return f"state incomplete: {miss}"
            if streamed and not (self.sweeps_ran and self.lists_on_host):
                return "a streamed call needs resident alphas and lists known to the host"
            return None
        return f"unknown op {name}"

    # ---- ops -----------------------------------------------------------------------------------------------------------------
    def apply(self, op, e=None):
        """Mutates the shadow as the header says the call mutates a context and, given an engine, makes the call(s).  An observe op
        returns what it downloaded."""
        why = self.illegal(op)
        if why:
            raise Illegal(f"{op}: {why}")
        rng = np.random.default_rng(op.get("seed", 0))
        return getattr(self, "_op_" + op["op"])(op, rng, e)

    def _keypoints_replaced(self, traj, update=False):
        """New lists for `traj`: a payload laid out by entry survives kpilqr_update_keypoints (the listed ranges pending) and is dropped
        by new lists for everybody; job lists carry indices of the OLD lists, where the header defines no result: a whole upload has
        to follow."""
        if update and self.payload in ("fd_kp", "cols"):
            self.pending = list(traj)
        else:
            self.payload, self.pending = "none", []
        self.lists_on_host = True

    def _op_set_keypoints(self, op, rng, e):
        shared = self._draw_rows(rng, op["how"]) if op["how"] != "bisect" else None
        self.rows = [shared if shared is not None else self._draw_rows(rng, "bisect") for _ in range(BATCH)]
        self._keypoints_replaced(range(BATCH))
        if e:
            e.set_keypoints_rows(self.rows)

    def _op_generate_keypoints(self, op, rng, e):
        dof, _, T, _ = self.dims
        if op["method"] == "set_interval":
            min_N = int(rng.choice([2, 4, 6]))
            self.rows = [orc.kp_set_interval(dof, T, min_N)] * BATCH
            args = ("set_interval", min_N, 1, None, 0.0)
        else:
            X = np.stack([_kp_states(rng, dof, T) for _ in range(BATCH)])
            thr = rng.uniform(0.5, 20.0, dof)
            self.rows = [orc.kp_velocity_change(dof, T, 2, 12, thr, X[b]) for b in range(BATCH)]
            args = ("velocity_change", 2, 12, thr, 0.01)
        # (the oracle's rows may name a DoF twice at a step -- the last one, which every method fills --; the lists are the same, and
        # the FD jobs drawn from the rows must not come twice)
        o, t = rows_to_dof_csr(self.rows, dof, T)
        self.rows = [synth.rows_from_dof_lists(dof, T, [t[o[b * dof + i]:o[b * dof + i + 1]] for i in range(dof)]) for b in range(BATCH)]
        self._keypoints_replaced(range(BATCH))
        self.lists_on_host = False                 # the lists exist on the device only
        if e:
            if op["method"] != "set_interval":
                e.upload_states(X)
            e.generate_keypoints(*args)

    def _op_update_keypoints(self, op, rng, e):
        traj = SUBSETS[op["subset"]]
        if op["subset"] == "pair":                 # the first shrinks to the ends, the second grows to every step: kept ranges move both ways
            new = [self._draw_rows(rng, "ends"), self._draw_rows(rng, "every")]
        else:
            new = [self._draw_rows(rng, "bisect") for _ in traj]
        if traj:
            self.rows = list(self.rows)
            for b, rw in zip(traj, new):
                self.rows[b] = rw
            self._keypoints_replaced(traj, update=True)
        if e:
            e.update_keypoints_rows(traj, new)

    def _payload_arrays(self, p, traj=None):
        xp, xm, md = synth.kp_ordered_payload(p)
        if traj is not None:
            idx = _entries_of(p, traj)
            xp, xm, md = xp[idx], xm[idx], md[idx]
        return xp, xm, md

    def _upload_whole(self, e, p, how):
        if how == "jobs":
            e.upload_fd(p["job_b"], p["job_t"], p["job_col"], p["job_mode"], p["xplus"], p["xminus"], job_nom=p["job_nom"], xnom=p["xnom"], eps=EPS)
        elif how == "jobs_slab":
            e.upload_fd_slab(e.fd_slab(p["job_b"], p["job_t"], p["job_col"], p["job_mode"], p["xplus"], p["xminus"], p["job_nom"], p["xnom"]), EPS)
        elif how == "fd_kp":
            e.upload_fd_kp(e.fd_kp_slab(*self._payload_arrays(p)), eps=EPS)
        else:
            e.upload_kp_columns(e.kp_columns(*self._payload_arrays(p), eps=EPS))

    def _op_upload_payload(self, op, rng, e):
        self._new_payload_cfg(rng, range(BATCH))
        self.payload, self.pending = op["kind"].replace("_slab", ""), []
        if e:
            self._upload_whole(e, self.problem(), op["kind"])

    def _op_upload_payload_partial(self, op, rng, e):
        traj, self.pending = self.pending, []
        self._new_payload_cfg(rng, traj)
        if e:
            arr = self._payload_arrays(self.problem(), traj)
            if self.payload == "fd_kp":
                e.upload_fd_kp_partial(traj, e.fd_kp_slab(*arr), eps=EPS)
            else:
                e.upload_kp_columns_partial(traj, e.kp_columns(*arr, eps=EPS))

    def _op_upload_residuals(self, op, rng, e):
        r, r_x, r_u = self._draw_residuals(rng, BATCH, op["what"])
        self.r, self.have_r = r, True
        if r_x is not None:
            self.r_x, self.rx_mode, self.rx_whole = r_x, "step", True
        if r_u is not None:
            self.r_u, self.ru_written = r_u, True
        if e:
            e.upload_residuals(r, r_x, r_u, None, None)

    def _op_rx_const(self, op, rng, e):
        _, m, T, nr = self.dims
        self.rx_mode, self.rx_whole = "const", False
        self.r_x = np.broadcast_to(self.rx_const, self.r_x.shape).copy()
        self.r_u, self.ru_written = np.zeros_like(self.r_u), False      # r_u = NULL: the buffer is zeroed, the r_u-free sweeps run again
        if e:
            e.upload_residual_jacobians_const(self.rx_const, None)

    def _op_residuals_partial(self, op, rng, e):
        traj = op["subset"]
        r, r_x, r_u = self._draw_residuals(rng, len(traj), op["what"])
        self.r = self.r.copy(); self.r[traj] = r
        if r_x is not None:
            self.r_x = self.r_x.copy(); self.r_x[traj] = r_x
        if r_u is not None:
            self.r_u = self.r_u.copy(); self.r_u[traj] = r_u
        if e:
            e.upload_residuals_partial(traj, r, r_x, r_u)

    def _op_nominal(self, op, rng, e):
        """New controls and limits tight enough that the clamp is active on some controls of every trajectory: the nominal controls
        reach 0.3 of the actuator range, the limits 0.15 to 0.25 of it."""
        _, m, T, _ = self.dims
        lim = np.asarray(self.cfg["lim"], float)
        self.u_nom = rng.uniform(-0.3, 0.3, (BATCH, T, m)) * lim[None, None, :]
        tight = lim * rng.uniform(0.15, 0.25)
        self.ctrl_lim = np.stack([-tight, tight], axis=1).reshape(-1)
        self.have_nom = True
        if e:
            e.upload_nominal(self.u_nom, self.ctrl_lim)

    def _op_nominal_partial(self, op, rng, e):
        _, m, T, _ = self.dims
        traj = op["subset"]
        u = rng.uniform(-0.3, 0.3, (len(traj), T, m)) * np.asarray(self.cfg["lim"], float)[None, None, :]
        self.u_nom = self.u_nom.copy(); self.u_nom[traj] = u
        if e:
            e.upload_nominal_partial(traj, u)

    def _op_weights(self, op, rng, e):
        nr = self.dims[3]
        self.w_run = np.asarray(self.cfg["w_run"], float) * rng.uniform(0.5, 2.0, nr)
        self.w_term = np.asarray(self.cfg["w_term"], float) * rng.uniform(0.5, 2.0, nr)
        assert np.all(self.w_run > 0) and np.all(self.w_term > 0)
        if e:
            e.upload_residuals(None, None, None, self.w_run, self.w_term)

    def _op_lam(self, op, rng, e):
        self.lam = 10.0 ** rng.uniform(-2.0, 1.0, BATCH)           # goes to the device with the next sweep

    def _op_resize(self, op, rng, e):
        self.shape ^= 1
        self.n_resize += 1
        self._forget()
        if e:
            dof, m, T, _ = self.dims
            e.resize(dof, m, T)

    def _op_stage(self, op, rng, e):
        """Explicit stage calls and read-backs: none may change a result."""
        call = op["call"]
        if call == "device_ptr_rx":                # a writable pointer leaves the library: the broadcast copy is made, the constant mode ends
            self.rx_mode, self.rx_whole = "step", True
        if call == "get_keypoints":
            self.lists_on_host = True
        if not e:
            return
        if call in ("fd_difference", "interpolate", "fd_interpolate", "cost_derivs", "get_AB", "get_union_columns", "backward_stats"):
            getattr(e, call)()
        elif call in ("fd_interpolate_partial", "cost_derivs_partial"):
            # in the listed records bit for bit what the whole-batch call writes there, no byte of anybody else's records written
            whole, get = (e.fd_interpolate, e.get_AB) if call == "fd_interpolate_partial" else (e.cost_derivs, e.get_cost_derivs)
            rest = [b for b in range(BATCH) if b not in op["subset"]]
            before = get()
            getattr(e, call)(op["subset"])
            after = get()
            whole()
            for x0, x1, x2 in zip(before, after, get()):
                # (job lists: k_fd_difference runs over the RESIDENT jobs, those of kept trajectories rewrite their key-point columns)
                if not (call == "fd_interpolate_partial" and self.payload == "jobs"):
                    assert np.array_equal(x1[rest], x0[rest]), (call, "records of a trajectory that is not listed were written")
                assert np.array_equal(x1[op["subset"]], x2[op["subset"]]), (call, "not the records of the whole-batch call")
        elif call == "get_union_keypoints":
            offs, times = e.get_union_keypoints()
            o, t = rows_to_dof_csr(self.rows, self.dims[0], self.dims[2])
            for b in range(BATCH):                 # the union of a trajectory's per-DoF lists
                want = np.unique(t[o[b * self.dims[0]]:o[(b + 1) * self.dims[0]]])
                assert np.array_equal(times[offs[b]:offs[b + 1]], want), ("union lists", b)
        elif call == "device_ptr_rx":
            from trajoptkp_amd import _lib
            e.device_array(_lib.BUF_R_X, self.r_x.shape)
        elif call == "get_keypoints":
            o, t = e.get_keypoints()
            wo, wt = rows_to_dof_csr(self.rows, self.dims[0], self.dims[2])
            assert np.array_equal(o, wo) and np.array_equal(t, wt), "kpilqr_get_keypoints differs from the shadow's lists"
        elif call == "update_none":
            e.update_keypoints_rows([], [])

    def _op_refuse(self, op, rng, e):
        """A call the header documents as refused: the documented code, and (shown by the next observation) nothing changed."""
        if not e:
            return
        which = op["which"]
        dof, m, T, nr = self.dims

        def raises(code, call, *a, **kw):
            try:
                call(*a, **kw)
            except KpilqrError as err:
                assert err.code == code, (which, err.code, str(err))
                return
            raise AssertionError(f"{which}: the call was not refused")
        if which == "observe_pending":
            raises(ERR_STATE, e.iterate, self.lam, 100, ALPHAS)
        elif which == "update_pending":
            raises(ERR_STATE, e.update_keypoints_rows, [0], [self._draw_rows(rng, "ends")])
        elif which in ("rx_rows_const", "rx_rows_before_whole"):
            raises(ERR_STATE, e.upload_residuals_partial, [1], None, np.ones((1, T + 1, nr, 2 * dof)), None)
        elif which == "ru_rows_before_whole":
            raises(ERR_STATE, e.upload_residuals_partial, [BATCH - 1], None, None, np.ones((1, T + 1, nr, m)))
        elif which == "partial_records_fused":
            raises(ERR_STATE, e.fd_interpolate_partial, [0, 2])
            raises(ERR_STATE, e.cost_derivs_partial, [0, 2])
        else:
            wrong = [b for b in range(BATCH) if b not in self.pending] or self.pending[:-1]      # never the pending set
            arr = self._payload_arrays(self.problem(), wrong)
            if self.payload == "fd_kp":
                raises(ERR_ARG, e.upload_fd_kp_partial, wrong, e.fd_kp_slab(*arr), eps=EPS)
            else:
                raises(ERR_ARG, e.upload_kp_columns_partial, wrong, e.kp_columns(*arr, eps=EPS))

    # ---- observation ---------------------------------------------------------------------------------------------------------
    def _op_observe(self, op, rng, e):
        streamed = op["how"] == "streamed"
        new = {}
        if streamed and op.get("payload"):         # a whole new payload rides on the call: it completes pending ranges
            self._new_payload_cfg(rng, range(BATCH))
            self.payload, self.pending = op["payload"], []
        if streamed and op.get("res"):
            r, r_x, _ = self._draw_residuals(rng, BATCH, op["res"])
            self.r, self.have_r = r, True
            new["r"] = r
            if r_x is not None:                    # per-step Jacobians in the call end the constant mode
                self.r_x, self.rx_mode, self.rx_whole = r_x, "step", True
                new["r_x"] = r_x
        self.sweeps_ran = True
        return observe(e, self, op, new) if e else None


def _pin(e, a, dtype=None):
    a = np.asarray(a)
    out = e.pinned(a.shape, dtype or a.dtype)
    out[...] = a
    return out


def observe(e, sh, op, new=None):
    """The observe call of op on engine e (the sequence's context or a fresh one) and everything it downloads."""
    dof, m, T, nr = sh.dims
    n = 2 * dof
    how = op["how"]
    out = {}
    if how == "iterate":
        e.iterate(sh.lam, 100, ALPHAS)
        res = e.results()
        out.update(status=res["status"], delta_J=res["delta_J"], cost=res["cost_pred"])
    elif how == "staged":
        if not sh.fused:                           # a context with records: the stages kpilqr_iterate would run
            e.fd_interpolate()
            if not sh.a6:
                e.cost_derivs()
        out["status"], out["delta_J"] = e.backward(sh.lam, 100)
        out["cost"], out["U"] = e.forward_linear(ALPHAS, want_U=True)
    else:
        p = sh.problem()
        kw = {}
        if op.get("payload") == "jobs":
            kw["fd"] = e.fd_slab(p["job_b"], p["job_t"], p["job_col"], p["job_mode"], p["xplus"], p["xminus"], p["job_nom"], p["xnom"])
        elif op.get("payload") == "fd_kp":
            kw["fd_kp"] = e.fd_kp_slab(*sh._payload_arrays(p))
        elif op.get("payload") == "cols":
            kw["kp_cols"] = e.kp_columns(*sh._payload_arrays(p), eps=EPS)
        for name, a in (new or {}).items():
            kw[name] = _pin(e, a)
        K, k = e.pinned((BATCH, T, n, m)), e.pinned((BATCH, T, m))
        cp, dJ, st = e.pinned((BATCH, 6)), e.pinned(BATCH), e.pinned(BATCH, np.int32)
        st[:] = -1
        e.iterate_streamed(eps=EPS, lam=_pin(e, sh.lam), K=K, k=k, cost_pred=cp, delta_J=dJ, status=st, nchunks=op["nchunks"], **kw)
        e.sync()
        out.update(status=np.array(st), delta_J=np.array(dJ), cost=np.array(cp), K_streamed=np.array(K), k_streamed=np.array(k))
    launch = [e.last_launch("backward"), e.last_launch("forward")]
    out["linearise"] = e.last_launch("linearise")
    out["K"], out["k"] = e.gains()
    if how == "streamed":                          # the ordinary calls behind a streamed iteration see its results
        assert np.array_equal(out.pop("K_streamed"), out["K"]) and np.array_equal(out.pop("k_streamed"), out["k"]), "gains behind a streamed call"
    if how != "staged":                            # U_alpha comes from kpilqr_forward_linear alone: one more forward sweep on the same state
        out["cost_fwd"], out["U"] = e.forward_linear(ALPHAS, want_U=True)
        launch.append(e.last_launch("forward"))
    out["launch"] = tuple(launch)
    gains = op.get("gains", "all")
    if gains == "subset":
        Kp, kp = e.gains(traj=op["subset"])
        assert np.array_equal(Kp, out["K"][op["subset"]]) and np.array_equal(kp, out["k"][op["subset"]]), "gains of a subset"
    elif gains == "f32":                           # both conversions are round-to-nearest-even
        K32, k2 = e.gains(f32=True)
        assert K32.dtype == np.float32 and np.array_equal(K32, out["K"].astype(np.float32)) and np.array_equal(k2, out["k"]), "FP32 gains"
    if not sh.fused:
        out["A"], out["B"] = e.get_AB()
        if not sh.a6:                              # (a6: the cost derivatives are formed inside the sweeps, the records' are not current)
            out["l_x"], out["l_xx"], out["l_u"], out["l_uu"] = e.get_cost_derivs()
    return out


# ---- contexts -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _environ(env, setenv, delenv):
    for k, v in env.items():
        setenv(k, v)
    try:
        yield
    finally:
        for k in env:
            delenv(k)                              # read once, in kpilqr_create


def make_engine(sh, setenv=None, delenv=None):
    """An Engine of the shadow's kind at its current shape (environment set and removed around kpilqr_create)."""
    from trajoptkp_amd import Engine
    setenv = setenv or os.environ.__setitem__
    delenv = delenv or (lambda k: os.environ.pop(k, None))
    dof, m, T, nr = sh.dims
    with _environ(sh.K["env"], setenv, delenv):
        e = Engine(dof, m, T, nr, batch=BATCH, **sh.K["kw"])
    assert ("t1_fused" in e.backward_variant) == sh.fused and e.backward_variant.endswith("_a6") == sh.a6, (sh.kind, e.backward_variant)
    return e


def fresh_observation(sh, op, setenv=None, delenv=None):
    """The yardstick: a second context of the same kind and environment brought to the shadow's state by the shortest whole-batch
    route -- lists, one whole payload of the resident kind, one residual upload in the shadow's Jacobian mode (r_u iff it was ever
    written), the nominal controls -- and the same observe call."""
    p = sh.problem()
    new = {}
    if op["how"] == "streamed" and op.get("res"):
        new["r"] = sh.r
        if "rx" in op["res"]:
            new["r_x"] = sh.r_x
    with make_engine(sh, setenv, delenv) as f:
        f.set_keypoints_rows(p["kp_rows"])
        r_u = sh.r_u if sh.ru_written else None
        if sh.rx_mode == "const":
            f.upload_residual_jacobians_const(sh.rx_const, None)
            f.upload_residuals(sh.r, None, r_u, sh.w_run, sh.w_term)
        else:
            f.upload_residuals(sh.r, sh.r_x, r_u, sh.w_run, sh.w_term)
        f.upload_nominal(sh.u_nom, sh.ctrl_lim)
        if op["how"] == "streamed":                # a streamed call takes the resident alphas (the sweep itself runs on no payload once)
            f.forward_linear(ALPHAS, fetch=False)
        sh._upload_whole(f, p, sh.payload)
        return observe(f, sh, op, new)


# ---- comparisons --------------------------------------------------------------------------------------------------------------
def oracle_errors(got, refs):
    """status equal; worst relative error per quantity over the batch."""
    worst = {}
    for b, o in enumerate(refs):
        assert o["status"] == 0 and got["status"][b] == 0, ("status", b, int(got["status"][b]), o["status"])
        errs = dict(K=_rel(got["K"][b], o["K"]), k=_rel(got["k"][b], o["k"]),
                    delta_J=abs(got["delta_J"][b] - o["delta_J"]) / max(abs(o["delta_J"]), 1e-300),
                    cost=_rel(got["cost"][b], o["cost_pred"]), U=_rel(got["U"][b], o["U_alpha"]))
        if "cost_fwd" in got:
            errs["cost"] = max(errs["cost"], _rel(got["cost_fwd"][b], o["cost_pred"]))
        for key, v in errs.items():
            worst[key] = max(worst.get(key, 0.0), v)
    return worst


def fresh_errors(got, want):
    """-> (bit_equal, worst relative difference).  Equal launch strings: every output np.array_equal (the caller asserts); other
    forms of the same sweeps: RTOL_FORMS.  The records of a context that has them are array_equal whatever the sweeps' form."""
    same_form = got["launch"] == want["launch"]
    worst = 0.0
    for key in want:
        if key in ("launch", "linearise"):
            continue
        if key in ("A", "B", "l_x", "l_xx", "l_u", "l_uu") or same_form:
            assert np.array_equal(got[key], want[key]), ("not the bytes of a fresh context", key, got["launch"], want["launch"])
        else:
            for b in range(BATCH):
                worst = max(worst, _rel(got[key][b], want[key][b]))
    return same_form, worst


# ---- generator ----------------------------------------------------------------------------------------------------------------
def op_class(op):
    """The class an op counts as in the coverage tables (one per bullet of the op list)."""
    name = op["op"]
    if name == "set_keypoints":
        return [f"set_keypoints:{op['how']}"]
    if name == "generate_keypoints":
        return ["generate_keypoints"]
    if name == "update_keypoints":
        return [f"update_keypoints:{op['subset']}"]
    if name == "upload_payload":
        return [f"payload:{op['kind']}"] + (["payload:new_under_unchanged_keypoints"] if op.get("same_kp") else [])
    if name == "upload_residuals":
        return [f"residuals:{op['what']}"]
    if name == "stage":
        return [f"stage:{op['call']}"]
    if name == "refuse":
        return [f"refuse:{op['which']}"]
    if name == "observe":
        out = [f"observe:{op['how']}", f"gains:{op.get('gains', 'all')}"]
        if op["how"] == "streamed":
            out += [f"streamed:nchunks{op['nchunks']}", f"streamed:payload_{op.get('payload') or 'none'}"]
            if op.get("res"):
                out.append(f"streamed:res_{op['res']}")
        return out
    return [name]


def classes_of(kind):
    """Every op class a kind has to show across its seeds."""
    sh = Shadow(kind)
    second = Shadow(kind); second.shape = 1
    fused_somewhere, records_somewhere = sh.fused or second.fused, not sh.fused or not second.fused
    out = [f"set_keypoints:{h}" for h in ("interval", "bisect", "every", "ends")] + ["generate_keypoints"]
    out += [f"update_keypoints:{s}" for s in ("first", "last", "pair", "all")]
    out += [f"payload:{k}" for k in ("jobs", "jobs_slab", "fd_kp", "cols")] + ["upload_payload_partial", "payload:new_under_unchanged_keypoints"]
    out += [f"residuals:{w}" for w in ("r", "r+rx", "r+rx+ru")] + ["rx_const", "residuals_partial", "nominal_partial", "nominal", "weights", "lam", "resize"]
    for call in STAGE_CALLS:
        if call in ("fd_interpolate_partial", "cost_derivs_partial") and not records_somewhere:
            continue
        if call in ("get_union_keypoints", "get_union_columns") and not sh.union:
            continue
        if call == "backward_stats" and not fused_somewhere:
            continue
        out.append(f"stage:{call}")
    out += [f"observe:{h}" for h in ("iterate", "staged", "streamed")] + [f"gains:{g}" for g in ("all", "subset", "f32")]
    out += [f"streamed:nchunks{c}" for c in (1, 2, 3)] + [f"streamed:payload_{k}" for k in ("none", "jobs", "fd_kp", "cols")]
    return out


def draw_sequence(rng, kind, n_ops=N_OPS, min_obs=MIN_OBS):
    """A list of n_ops ops, legal by the header, with at least min_obs observations.  It proceeds in rounds -- a few changes (or a
    stretch of explicit stage calls alone), whatever uploads the header requires before the next sweep, sometimes a documented
    refusal, then an observation -- and never observes where the header defines no result (key-points but no payload ...).  Classes
    are dealt from a shuffled deck, so that one sequence repeats a class only after it has shown all the others."""
    sh = Shadow(kind)
    ops, n_obs = [], 0
    seed = lambda: int(rng.integers(1, 1 << 30))
    decks = {}

    def deal(name, items):
        if not decks.get(name):
            decks[name] = list(rng.permutation(np.asarray(items, dtype=object)))
        return decks[name].pop()

    def subset():
        return sorted(int(b) for b in rng.choice(BATCH, size=int(rng.integers(1, BATCH)), replace=False))

    def per_dof_biased(hows):
        # a union context takes its route on per-DoF lists only: most key-point ops draw those
        return "bisect" if sh.union and rng.uniform() < 0.6 else deal("kp_how", hows)

    def change(s):
        """One op that changes a result (or a state the results depend on)."""
        # (partial re-linearisation is what the real caller does most: it is dealt three times as often)
        menu = ["set_keypoints", "generate_keypoints", "update_keypoints", "upload_payload", "upload_residuals", "rx_const", "residuals_partial",
                "nominal_partial", "nominal", "weights", "lam", "update_keypoints", "update_keypoints", "upload_payload", "set_keypoints"]
        while True:
            name = deal("change", menu)
            if name == "set_keypoints":
                op = dict(op=name, how=per_dof_biased(["interval", "bisect", "every", "ends"]), seed=seed())
            elif name == "generate_keypoints":
                op = dict(op=name, method="velocity_change" if sh.union or rng.uniform() < 0.7 else "set_interval", seed=seed())
            elif name == "update_keypoints":
                op = dict(op=name, subset=deal("update", ["first", "last", "pair", "all"]), seed=seed())
            elif name == "upload_payload":
                op = dict(op=name, kind=deal("payload", PAYLOAD_DECK), seed=seed(),
                          same_kp=s.payload != "none" and not s.pending)
            elif name == "upload_residuals":
                op = dict(op=name, what=deal("res", ["r", "r+rx", "r+rx+ru"]), seed=seed())
            elif name == "residuals_partial":
                what = "r" + ("+rx" if s.rx_mode == "step" and s.rx_whole and rng.uniform() < 0.7 else "") + ("+ru" if s.ru_written and rng.uniform() < 0.7 else "")
                op = dict(op=name, subset=subset(), what=what, seed=seed())
            elif name == "nominal_partial":
                op = dict(op=name, subset=subset(), seed=seed())
            else:
                op = dict(op=name, seed=seed())
            if not s.illegal(op):
                return op

    def fill(s):
        """The uploads the header requires before the next sweep, in the state s."""
        out = []
        while True:
            miss = s.missing()
            if not miss:
                return out
            what = miss[0]
            if what == "kp":
                op = dict(op="set_keypoints", how=per_dof_biased(["interval", "bisect", "every", "ends"]), seed=seed()) if rng.uniform() < 0.75 \
                    else dict(op="generate_keypoints", method="velocity_change" if s.union or rng.uniform() < 0.7 else "set_interval", seed=seed())
            elif what == "payload":
                op = dict(op="upload_payload", kind=deal("payload", PAYLOAD_DECK), seed=seed(), same_kp=False)
            elif what == "pending":
                op = dict(op="upload_payload_partial", seed=seed()) if rng.uniform() < 0.8 \
                    else dict(op="upload_payload", kind=deal("payload", PAYLOAD_DECK), seed=seed(), same_kp=False)
            elif what == "r":
                op = dict(op="upload_residuals", what=deal("res", ["r", "r+rx", "r+rx+ru"]), seed=seed())
            elif what == "rx":
                op = dict(op="rx_const", seed=seed()) if rng.uniform() < 0.4 else dict(op="upload_residuals", what=deal("res_rx", ["r+rx", "r+rx+ru"]), seed=seed())
            elif what == "w":
                op = dict(op="weights", seed=seed())
            else:
                op = dict(op="nominal", seed=seed())
            s.apply(op)
            out.append(op)

    def refusal(s):
        avail = [w for w in REFUSALS if not s.illegal(dict(op="refuse", which=w))]
        if not avail:
            return None
        rare = [w for w in avail if w in ("observe_pending", "update_pending", "partial_upload_wrong_traj", "rx_rows_before_whole")]
        want = deal("refuse", list(REFUSALS))
        return dict(op="refuse", which=want if want in avail else str(rng.choice(rare or avail)), seed=seed())

    def stage(s):
        avail = [c for c in STAGE_CALLS if not s.illegal(dict(op="stage", call=c, subset=[0]))]
        for _ in range(len(STAGE_CALLS)):
            call = deal("stage", list(STAGE_CALLS))
            if call in avail:
                break
        else:
            call = str(rng.choice(avail))
        op = dict(op="stage", call=call)
        if call.endswith("_partial"):
            op["subset"] = subset()
        return op

    def observation(s):
        """An observe op legal in s; a streamed one may bring the payload (and residuals) that are still missing."""
        how = deal("how", ["iterate", "staged", "streamed", "streamed"])
        op = dict(op="observe", how=how, gains=deal("gains", ["all", "subset", "f32"]), seed=seed())
        if op["gains"] == "subset":
            op["subset"] = subset()
        if how == "streamed":
            op.update(nchunks=int(deal("nchunks", [1, 2, 3])), payload=deal("spay", [None, None, "jobs", "fd_kp", "cols"]),
                      res=deal("sres", [None, None, "r", "r+rx"]))
            if s.illegal(op):
                op = dict(op="observe", how=deal("plain", ["iterate", "staged"]), gains=op["gains"], seed=op["seed"], **({"subset": op["subset"]} if "subset" in op else {}))
        return op

    def round_(extras):
        """One round on a copy of the shadow: -> its ops.  extras: how many ops beyond the required ones it may spend."""
        s = copy.deepcopy(sh)
        out = []

        def emit(op):
            s.apply(op)
            out.append(op)
        complete = not s.missing()
        if complete and extras >= 1 and rng.uniform() < 0.25:                # a stretch of explicit stage calls alone
            for _ in range(int(rng.integers(1, min(extras, 3) + 1))):
                emit(stage(s))
        else:
            if extras >= 9 and s.sweeps_ran and rng.uniform() < (0.5 if s.n_resize % 2 else 0.15):
                emit(dict(op="resize"))
                extras -= 7
            n_change = 0 if extras < 2 else int(rng.integers(1, min(extras // 2, 2) + 1))      # (a change may call for an upload of its own)
            for _ in range(n_change):
                emit(change(s))
            extras -= 2 * n_change
            if extras >= 1 and rng.uniform() < 0.45:
                op = refusal(s)
                if op:
                    emit(op)
                    extras -= 1
            # a streamed observation may bring what is missing itself; otherwise it is uploaded first
            ob = observation(s)
            if ob["how"] == "streamed" and not s.illegal(ob):
                emit(ob)
                return out
            out += fill(s)
            if extras >= 1 and rng.uniform() < 0.3:                          # stage calls between a change and its observation
                emit(stage(s))
            if s.illegal(ob):
                ob = observation(s)
            emit(ob)
            return out
        emit(observation(s))
        return out

    while len(ops) < n_ops:
        left = n_ops - len(ops)
        need = max(0, min_obs - n_obs)
        s = copy.deepcopy(sh)
        required = len(fill(s)) + 1
        extras = left - required - max(0, need - 1) * 2
        state = rng.bit_generator.state
        saved = copy.deepcopy(decks)
        rnd = round_(max(0, extras))
        if len(rnd) > left:                        # no room for it: the required uploads and the observation alone, else harmless ops
            rng.bit_generator.state = state
            decks.clear(); decks.update(saved)
            rnd = round_(0) if required <= left else []
            if not rnd or len(rnd) > left:
                rnd = [dict(op="lam", seed=seed()) for _ in range(left)]
        for op in rnd:
            sh.apply(op)
            ops.append(op)
            n_obs += op["op"] == "observe"
    assert len(ops) == n_ops and n_obs >= min_obs, (kind, len(ops), n_obs)
    return ops


@functools.lru_cache(maxsize=None)
def committed_sequence(kind, seed):
    # (the kind enters the stream so that two kinds do not walk the same decisions)
    return draw_sequence(np.random.default_rng([seed, sorted(KINDS).index(kind)]), kind)


def format_ops(ops):
    return "[\n" + "".join(f"    {op!r},\n" for op in ops) + "]"


# ---- running a sequence on the GPU ----------------------------------------------------------------------------------------------
def run_sequence(kind, ops, setenv=None, delenv=None, tag=""):
    """Applies ops to one context and its shadow; at every observation the results must match the oracle (RTOL) and a fresh context
    (bit for bit where both ran the same forms, RTOL_FORMS otherwise).  -> a summary dict."""
    sh = Shadow(kind)
    stats = dict(observations=0, launches=set(), worst={}, bit_equal=0, form_compared=0, worst_forms=0.0, per_launch={})
    with make_engine(sh, setenv, delenv) as e:
        for i, op in enumerate(ops):
            try:
                got = sh.apply(op, e)
                if op["op"] != "observe":
                    continue
                errs = oracle_errors(got, sh.oracle())
                assert max(errs.values()) <= RTOL, ("oracle", got["launch"], errs)
                same, diff = fresh_errors(got, fresh_observation(sh, op, setenv, delenv))
                assert diff <= RTOL_FORMS, ("fresh context", got["launch"], diff)
            except Exception as err:
                raise AssertionError(f"{tag or kind}: op {i} {op!r} failed: {err!r}\nthe sequence up to it:\n{format_ops(ops[:i + 1])}") from err
            stats["observations"] += 1
            stats["launches"].add(got["launch"][0])
            stats["bit_equal"] += same
            stats["form_compared"] += not same
            stats["worst_forms"] = max(stats["worst_forms"], diff)
            per = stats["per_launch"].setdefault(got["launch"][0], {})
            for key, v in errs.items():
                stats["worst"][key] = max(stats["worst"].get(key, 0.0), v)
                per[key] = max(per.get(key, 0.0), v)
    return stats
