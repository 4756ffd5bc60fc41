"""Shared by tests/test_gpu_streamed_subset.py: the small shapes, contexts and output checks of tests/test_gpu_streamed_columns_f32.py
(imported from there, not copied), two data sets per shape, their mixtures, and the yardstick of kpilqr_iterate_streamed4 with
upload_traj -- kpilqr_iterate_streamed3 on whole-batch arrays that hold data set A with the listed rows / entries replaced by B's.

Data set A is the problem as it is; B keeps the key-point lists and has the payload scaled as columns(name, scale=0.75) does (the x+- records:
x+ moved towards x- by the same factor) and r, r_x, u_nom perturbed.  Payload kinds: "cols" (FP64 columns), "cols32" (encoded FP32
columns), "fd_kp" (key-point ordered x+- records)."""
import ctypes as C

import numpy as np

import _columns_f32 as cf
from test_gpu_streamed_columns_f32 import (CONTEXTS, IDS, LISTS, OUT, Outputs, cast, check, chunk_counts, columns, engine, problem,   # noqa: F401
                                           relerr, same, setup, taken, TIGHT)
from trajoptkp_amd import _lib, synth

KINDS = ("cols", "cols32", "fd_kp")
ROWS = ("r", "r_x", "r_u", "u_nom")
SCALE_B = 0.75


def first_entries(p):
    """first CSR entry of every trajectory, [batch + 1]"""
    return np.asarray(cf.entry_csr(p)[0][::p["dof"]], np.int64)


def entry_index(p, traj):
    """the CSR entries of the listed trajectories, in list order"""
    f = first_entries(p)
    return np.concatenate([np.arange(f[b], f[b + 1]) for b in traj] + [np.zeros(0, np.int64)]).astype(np.int64)


def rows_of(p, which):
    """the per-trajectory inputs of data set A / B, float64 [batch][...]"""
    a = dict((k, np.array(p[k], np.float64)) for k in ROWS)
    if which == "B":
        a["r"] = a["r"] * 1.01 + 0.003
        a["r_x"] = a["r_x"] * 0.98
        a["u_nom"] = a["u_nom"] * 0.97 + 0.01
    return a


def payload_of(name, p, kind, which, every_step=(4,)):
    """the by-entry payload of data set A / B as arrays indexed by entry: a tuple that mix_payload / pin_payload understand"""
    scale = 1.0 if which == "A" else SCALE_B
    if kind == "cols":
        return (columns(name, scale, True, every_step)[0].copy(),)
    if kind == "cols32":
        return (columns(name, scale, True, every_step)[1].copy(),)
    xp, xm, mode = synth.kp_ordered_payload(p)
    return (xm + scale * (xp - xm), xm, mode)


def take(arrays, idx):
    return tuple(a[idx] for a in arrays)


def mix(a, b, idx):
    """a with the rows idx replaced by b's"""
    out = tuple(x.copy() for x in a)
    for x, y in zip(out, b):
        x[idx] = y[idx]
    return out


def pin_rows(e, rows, traj=None):
    """pinned copies of the per-trajectory inputs: whole, or the listed trajectories' rows back to back"""
    got = {}
    for k, a in rows.items():
        a = a if traj is None else a[np.asarray(traj, np.int64)]
        got[k] = e.pinned((max(len(a), 1),) + a.shape[1:])[:len(a)]
        got[k][...] = a
    return got


def pin_payload(e, kind, arrays):
    """the keyword of Engine.iterate_streamed3 / 4 that carries the payload"""
    if kind == "cols":
        a = e.pinned(max(arrays[0].size, 1)); a[:arrays[0].size] = arrays[0].reshape(-1)
        return dict(kp_cols=dict(cols=a, entries=len(arrays[0])))
    if kind == "cols32":
        a = e.pinned(max(arrays[0].size, 1), np.float32); a[:arrays[0].size] = arrays[0].reshape(-1)
        return dict(kp_cols32=a[:arrays[0].size])
    return dict(fd_kp=e.fd_kp_slab(*arrays))


def lam_of(e, p):
    lam = e.pinned(p["batch"]); lam[:] = p["lam"]
    return lam


def call(e, out, nchunks, lam, eps, upload_traj=None, gain=None, f32=False, four=True, **inputs):
    """Engine.iterate_streamed4 (four=False: iterate_streamed3) into `out`, no wait"""
    v = out.view
    kw = dict(K=None if f32 else v["K"], k=v["k"], cost_pred=v["cost_pred"], delta_J=v["delta_J"], status=v["status"], nchunks=nchunks,
              K32=v["K32"] if f32 else None, gain_traj=gain, lam=lam, eps=eps, **inputs)
    if four:
        e.iterate_streamed4(upload_traj=upload_traj, **kw)
    else:
        assert upload_traj is None
        e.iterate_streamed3(**kw)


def launches(e):
    return [e.last_launch(w) for w in ("backward", "forward", "linearise")]


class Yardstick:
    """ONE fresh context per (shape, family, payload kind) that only ever runs kpilqr_iterate_streamed3 (three chunks) on whole-batch
    arrays: every call replaces every input, so a call's outputs are those of a context that has seen nothing else."""

    def __init__(self, name, fused, kind, p=None, every_step=(4,), retry=None, pd_stride=100):
        self.name, self.kind, self.every_step, self.pd_stride = name, kind, every_step, pd_stride
        self.p = problem(name, True, every_step) if p is None else p
        self.e = engine(self.p, fused)
        setup(self.e, self.p)
        if retry:
            self.e.set_lambda_retry(**retry)
        self.lam = lam_of(self.e, self.p)
        self.memo = {}

    def close(self):
        self.e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def run(self, rows, pay, lam=None):
        """outputs (and launch strings) of the whole call on these arrays (pay = None: no payload, the resident one is swept again)"""
        e = self.e
        if lam is not None:
            self.lam[:] = lam
        out = Outputs(e)
        call(e, out, 3, self.lam, self.p["eps"], four=False, pd_stride=self.pd_stride, **pin_rows(e, rows), **({} if pay is None else pin_payload(e, self.kind, pay)))
        e.sync()
        ref = taken(out)
        ref["launch"] = launches(e)
        return ref

    def mixed(self, pay_list, row_list):
        """data set A with B's payload entries for pay_list and B's rows for row_list (None: nobody's)"""
        key = (None if pay_list is None else tuple(pay_list), None if row_list is None else tuple(row_list))
        if key not in self.memo:
            p = self.p
            pay = payload_of(self.name, p, self.kind, "A", self.every_step)
            if pay_list is not None:
                pay = mix(pay, payload_of(self.name, p, self.kind, "B", self.every_step), entry_index(p, pay_list))
            rows = rows_of(p, "A")
            if row_list is not None:
                rb, idx = rows_of(p, "B"), np.asarray(row_list, np.int64)
                for k in rows:
                    rows[k][idx] = rb[k][idx]
            ref = self.run(rows, pay)
            ref["rows"], ref["pay"] = rows, pay
            self.memo[key] = ref
        return self.memo[key]


def hold_to_oracle(p, rows, cols, got, what):
    """K, k of every trajectory whose oracle status is 0 at the suite's 1e-9 against the C oracle on these rows and FP64 columns"""
    q = dict(p)
    q.update(rows)
    held = 0
    for b in range(p["batch"]):
        o = cf.oracle_on_columns(q, cols, b, p["lam"])
        if o["status"] != 0:
            continue
        assert got["status"][b] == 0, (what, b)
        eK, ek = relerr(got["K"][b], o["K"]), relerr(got["k"][b], o["k"])
        print(f"{what} b={b}: K {eK:.2e} k {ek:.2e} against the oracle")
        assert eK < TIGHT and ek < TIGHT, (what, b, eK, ek)
        held += 1
    return held


def decoded_columns(name, p, kind, pay, every_step=(4,)):
    """the FP64 columns the device works on for a column payload (None for the x+- records: their differencing is held elsewhere)"""
    if kind == "cols":
        return pay[0]
    if kind == "cols32":
        return synth.decode_kp_columns_f32(pay[0], columns(name, 1.0, True, every_step)[3], p["dof"])
    return None


def raw_io4(e, out, lam, eps, rows=None, traj=None, kind=None, pay=None, entries=0):
    """kpilqr_stream_io4 with the standard outputs; rows / pay: what pin_rows / pin_payload returned.  The caller keeps `traj` alive."""
    io4 = _lib.StreamIO4()
    io4.struct_size = C.sizeof(_lib.StreamIO4)
    io4.io3.struct_size = C.sizeof(_lib.StreamIO3)
    io4.io3.io2.struct_size = C.sizeof(_lib.StreamIO2)
    io = io4.io3.io2.io
    io.eps = float(eps); io.entries = entries
    for k, a in (rows or {}).items():
        setattr(io, k, a.ctypes.data)
    io.lam = lam.ctypes.data
    if pay:
        if "kp_cols" in pay:
            io.kp_columns = pay["kp_cols"]["cols"].ctypes.data
        elif "kp_cols32" in pay:
            io4.io3.kp_columns32 = pay["kp_cols32"].ctypes.data
        else:
            io.fd_kp_slab = pay["fd_kp"]["slab"].ctypes.data
    for k in OUT:
        setattr(io, k, out.view[k].ctypes.data)
    if traj is not None:
        io4.upload_count = len(traj)
        io4.upload_traj = traj.ctypes.data
    return io4
