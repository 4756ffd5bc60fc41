"""GPU tests of kpilqr_iterate_streamed3 (csrc/columns_f32.hip: launch_kp_columns_f32_range): the chunk pipeline taking the key-point
columns as ENCODED FP32 -- one upload of a chunk's floats into its range of the context's staging buffer, one launch that decodes
that range into the chunk's range of the column store.

The yardstick is never the code under test: the reference of a shape is ONE kpilqr_iterate_streamed run (three chunks) on a fresh
context, fed the numpy-DECODED doubles (synth.decode_kp_columns_f32) as FP64 kp_columns; K, k, cost_pred, delta_J and status of the new
call must be its bits.  K and k are also held to the C oracle run on the decoded columns at the suite's 1e-9, and on every shape more
than 1/8 of the decoded elements differ from the FP64 columns (the test is not FP64 in disguise).

Shapes (the smallest at which the chunk indexing can go wrong; min_N = 5, dense residuals):
  panda7     panda_reaching T = 17, batch 7, fused     35 entries each; 3n = 42 floats per entry: a chunk's float range is 8- but not
                                                       16-byte aligned
  acrobot3   acrobot        T = 5,  batch 3, fused     4 entries each; m < dof: the kind-2 slots of DoF 1 carry 3.25 and are ignored
  panda5rec  panda_reaching T = 17, batch 5, on a context with step records
  pushing3   panda_pushing  T = 17, batch 3, tiled     50 entries each
  ragged5    panda_reaching T = 40, batch 5, fused and records; lists [bisected seed 21, the {0, 39} minimum, bisected 23, bisected 24,
                                                       every step]: 104, 14, 73, 78, 280 entries, three chunks carry 104 | 87 | 358
On the CPU oracle, on panda7, acrobot3, pushing3 and ragged5: status 0 for every trajectory on the decoded and on the FP64 columns,
and the FP32 transport moves K by at most 4.8e-8 relative (panda5rec is panda7's recipe at batch 5).
Every output lies inside a larger pinned allocation between 64 sentinel elements."""
import ctypes as C
import functools

import numpy as np
import pytest

import _columns_f32 as cf
from oracle import oracle as orc
from trajoptkp_amd import Engine, _lib, synth

pytestmark = pytest.mark.gpu

PAD = 64
TIGHT = 1e-9
SENT = {np.dtype(np.float64): -7.25, np.dtype(np.float32): np.float32(-7.25), np.dtype(np.int32): np.int32(-77)}
SHAPES = {      # name: (task, T, batch)
    "panda7": ("panda_reaching", 17, 7),
    "acrobot3": ("acrobot", 5, 3),
    "panda5rec": ("panda_reaching", 17, 5),
    "pushing3": ("panda_pushing", 17, 3),
    "ragged5": ("panda_reaching", 40, 5),
}
CONTEXTS = [("panda7", True), ("acrobot3", True), ("panda5rec", False), ("pushing3", False), ("ragged5", True), ("ragged5", False)]
IDS = [f"{n}-{'fused' if f else 'records'}" for n, f in CONTEXTS]
ENTRIES = {"panda7": [35] * 7, "acrobot3": [4] * 3, "panda5rec": [35] * 5, "pushing3": [50] * 3, "ragged5": [104, 14, 73, 78, 280]}
OUT = ("K", "k", "cost_pred", "delta_J", "status")
# Gains of a list (with three chunks; the lists of tests/test_gpu_streamed_gains.py): first | last | straddling a chunk boundary | nobody
LISTS = {7: [[0], [6], [1, 2], []], 5: [[0], [4], [0, 1], []], 3: [[0], [2], [0, 1], []]}


def cast(K):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(K, np.float64).astype(np.float32)


def same(got, want):
    """bit for bit"""
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(u), want.view(u))


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(float(np.max(np.abs(b))), 1e-300))


# ---- problems and their columns ----------------------------------------------------------------------------------------------------
def _by_entry(p):
    """Control columns without a DoF list (m > dof) have no slot in a by-entry payload: dropped, so that the oracle sees the same jobs"""
    keep = p["job_col"] < p["n"] + min(p["m"], p["dof"])
    q = dict(p)
    for k in ("job_b", "job_t", "job_col", "job_mode", "job_nom", "xplus", "xminus"):
        q[k] = p[k][keep]
    return q


def _bisected(dof, T, seed):
    rng = np.random.default_rng(seed)
    return synth.bisect_keypoints(rng, dof, T, 1, rng.uniform(0.2, 1.0, dof))


def ragged_rows(every_step=(4,)):
    """the lists of ragged5; every_step: the trajectories whose DoFs have a key-point at every step"""
    dof, T = 7, 40
    rows = [_bisected(dof, T, 21), synth.rows_from_dof_lists(dof, T, [[0, T - 1]] * dof), _bisected(dof, T, 23), _bisected(dof, T, 24), None]
    for b in every_step:
        rows[b] = synth.rows_from_dof_lists(dof, T, [list(range(T))] * dof)
    return rows


@functools.lru_cache(maxsize=None)
def problem(name, dense=True, every_step=(4,)):
    task, T, batch = SHAPES[name]
    if name == "ragged5":
        p = _by_entry(synth.make_ragged_problem(task, T, ragged_rows(every_step), config_id=7, one_sided_frac=0.2))
    else:
        p = _by_entry(synth.make_problem(task=task, T=T, batch=batch, min_N=5, dense_residuals=dense))
    assert p["batch"] == batch
    return p


@functools.lru_cache(maxsize=None)
def columns(name, scale=1.0, dense=True, every_step=(4,)):
    """(FP64 columns, encoded floats, decoded doubles, DoF of every entry) of a shape; the ignored kind-2 slots (DoFs >= m) carry a value
    of their own.  scale != 1: another payload on the same lists -- the O(dt) part (the columns without A's unit entry) scaled."""
    p = problem(name, dense, every_step)
    cols = synth.kp_columns(p)
    dofs = synth.kp_entry_dofs(p)
    if scale != 1.0:
        unit = synth._kp_unit_rows(dofs, p["dof"])
        cols[unit] -= 1.0
        cols *= scale
        cols[unit] += 1.0
    cols[dofs >= p["m"], 2, :] = 3.25
    c32 = synth.encode_kp_columns_f32(cols, dofs, p["dof"])
    dec = synth.decode_kp_columns_f32(c32, dofs, p["dof"])
    assert np.count_nonzero(dec != cols) > cols.size // 8          # the transport rounds: this is not the FP64 payload again
    return cols, c32, dec, dofs


def test_shapes_have_the_entries_the_chunks_are_cut_by():
    for name, want in ENTRIES.items():
        p = problem(name)
        offs, _ = cf.entry_csr(p)
        per = np.diff(offs[::p["dof"]])
        assert list(per) == want, (name, list(per))
    assert (3 * problem("panda7")["n"] * 4 * 35 * 3) % 16 == 8    # chunk [3, 7) of panda7 (two chunks) starts 8 mod 16 bytes into the staging buffer
    assert problem("acrobot3")["m"] < problem("acrobot3")["dof"]


# ---- contexts, inputs, outputs ------------------------------------------------------------------------------------------------------
def engine(p, fused):
    return Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=fused)


def setup(e, p, residual_jacobians=True):
    """Everything a streamed iteration needs beside its payload and outputs; returns the pinned per-iteration inputs"""
    e.set_keypoints_rows(p["kp_rows"])
    e.upload_residuals(None, None, None, p["w_run"], p["w_term"])
    e.upload_nominal(None, p["ctrl_lim"])
    e.forward_linear(orc.alphas(6), fetch=False)                  # (the alphas)
    return inputs(e, p, residual_jacobians)


def inputs(e, p, residual_jacobians=True):
    """the pinned per-iteration inputs of a problem"""
    inp = dict(eps=p["eps"])
    for name in ("r", "r_x", "r_u", "u_nom") if residual_jacobians else ("r", "u_nom"):
        inp[name] = e.pinned(p[name].shape); inp[name][...] = p[name]
    inp["lam"] = e.pinned(p["batch"]); inp["lam"][:] = p["lam"]
    return inp


def pin32(e, c32):
    a = e.pinned(max(c32.size, 1), np.float32)
    a[:c32.size] = c32.reshape(-1)
    return a[:c32.size]


def pin64(e, dec):
    a = e.pinned(max(dec.size, 1))
    a[:dec.size] = dec.reshape(-1)
    return dict(cols=a, entries=len(dec))


class Outputs:
    """One set of output buffers, each for the whole batch, inside a pinned allocation with PAD sentinel elements on both sides."""
    SPEC = (("K", np.float64, "perK"), ("K32", np.float32, "perK"), ("k", np.float64, "perk"), ("cost_pred", np.float64, "na"),
            ("delta_J", np.float64, "one"), ("status", np.int32, "one"))

    def __init__(self, e):
        self.B = e.batch
        self.row = dict(perK=e.T * e.n * e.m, perk=e.T * e.m, na=e.n_alpha, one=1)
        self.shape = dict(K=(e.T, e.n, e.m), K32=(e.T, e.n, e.m), k=(e.T, e.m), cost_pred=(e.n_alpha,), delta_J=(), status=())
        self.buf, self.view = {}, {}
        for name, dt, per in self.SPEC:
            n = self.B * self.row[per]
            b = e.pinned(n + 2 * PAD, dt); b[:] = SENT[np.dtype(dt)]
            self.buf[name], self.view[name] = b, b[PAD:PAD + n]

    def rows(self, name, count=None):
        """the first `count` rows (default: the whole batch) of an output, and -- asserted -- sentinels everywhere else"""
        count = self.B if count is None else count
        b, s = self.buf[name], SENT[self.buf[name].dtype]
        per = self.row[dict((n, p) for n, _, p in self.SPEC)[name]]
        assert np.all(b[:PAD] == s) and np.all(b[-PAD:] == s), f"{name}: a sentinel around the output was overwritten"
        assert np.all(self.view[name][count * per:] == s), f"{name}: written beyond {count} rows"
        return self.view[name][:count * per].reshape((count,) + self.shape[name])

    def untouched(self, *names):
        for name in names or self.buf:
            assert np.all(self.buf[name] == SENT[self.buf[name].dtype]), f"{name}: an output that was not asked for was written"


def call3(e, inp, out, nchunks, cols32=None, traj=None, f32=False, **payload):
    """Engine.iterate_streamed3 into `out` (no wait): the payload is cols32 (pinned floats) or what `payload` names"""
    v = out.view
    e.iterate_streamed3(K=None if f32 else v["K"], k=v["k"], cost_pred=v["cost_pred"], delta_J=v["delta_J"], status=v["status"],
                        nchunks=nchunks, K32=v["K32"] if f32 else None, gain_traj=traj, kp_cols32=cols32, **payload, **inp)


def check(out, ref, traj=None, f32=False, what=""):
    """after sync(): the outputs of a call against a reference"""
    rows = np.arange(out.B) if traj is None else np.array(traj, np.int64)
    if f32:
        assert same(out.rows("K32", len(rows)), cast(ref["K"][rows])), (what, traj, "K32 is not the cast of K")
        out.untouched("K")
    else:
        assert same(out.rows("K", len(rows)), ref["K"][rows]), (what, traj, "K")
        out.untouched("K32")
    assert same(out.rows("k", len(rows)), ref["k"][rows]), (what, traj, "k")
    for name in ("cost_pred", "delta_J", "status"):               # whole-batch outputs whatever the list says
        assert same(out.rows(name), ref[name]), (what, traj, name)


def taken(out):
    return dict((n, out.rows(n).copy()) for n in OUT)


def raw_io3(e, inp, out, cols32, entries):
    """kpilqr_stream_io3 with the standard inputs and outputs and the FP32 columns; the caller changes fields before it calls"""
    io3 = _lib.StreamIO3()
    io3.struct_size = C.sizeof(_lib.StreamIO3)
    io3.io2.struct_size = C.sizeof(_lib.StreamIO2)
    io = io3.io2.io
    io.eps = float(inp["eps"]); io.entries = entries
    io3.kp_columns32 = cols32.ctypes.data
    for name in ("r", "r_x", "r_u", "u_nom", "lam"):
        if name in inp:
            setattr(io, name, inp[name].ctypes.data)
    for name in OUT:
        setattr(io, name, out.view[name].ctypes.data)
    return io3


_REF = {}


def reference(name, fused, scale=1.0, fp64=False, every_step=(4,)):
    """The outputs of ONE kpilqr_iterate_streamed (three chunks) on a fresh context fed the decoded doubles (fp64: the FP64 columns
    themselves) as kp_columns"""
    key = (name, fused, scale, fp64, every_step)
    if key not in _REF:
        p = problem(name, True, every_step)
        cols, _, dec, _ = columns(name, scale, True, every_step)
        with engine(p, fused) as e:
            inp = setup(e, p)
            out = Outputs(e)
            v = out.view
            e.iterate_streamed(kp_cols=pin64(e, cols if fp64 else dec), K=v["K"], k=v["k"], cost_pred=v["cost_pred"], delta_J=v["delta_J"],
                               status=v["status"], nchunks=3, **inp)
            e.sync()
            ref = taken(out)
            out.untouched("K32")
            ref["launch"] = [e.last_launch(w) for w in ("backward", "forward", "linearise")]
        assert np.all(ref["status"] == 0) and np.all(np.isfinite(ref["K"]))
        _REF[key] = ref
    return _REF[key]


def hold_to_oracle(p, dec, got, what):
    for b in range(p["batch"]):
        o = cf.oracle_on_columns(p, dec, b, p["lam"])
        assert o["status"] == 0 and got["status"][b] == 0
        eK, ek = relerr(got["K"][b], o["K"]), relerr(got["k"][b], o["k"])
        print(f"{what} b={b}: K {eK:.2e} k {ek:.2e} against the oracle on the decoded columns")
        assert eK < TIGHT and ek < TIGHT, (what, b, eK, ek)


def chunk_counts(batch):
    return sorted({min(c, batch) for c in (1, 2, 3, 5, batch)})      # (5: two chunks on one pipeline stream)


# ---- 1. the bits of the FP64 call on the decoded doubles, at every chunk count -----------------------------------------------------
@pytest.mark.parametrize("name,fused", CONTEXTS, ids=IDS)
def test_streamed_f32_columns_give_the_bits_of_fp64_columns_decoded(name, fused):
    p, ref = problem(name), reference(name, fused)
    _, c32, dec, _ = columns(name)
    for nchunks in chunk_counts(p["batch"]):
        with engine(p, fused) as e:
            inp = setup(e, p)
            out = Outputs(e)
            call3(e, inp, out, nchunks, pin32(e, c32))
            e.sync()
            check(out, ref, what=nchunks)
            assert [e.last_launch(w) for w in ("backward", "forward", "linearise")] == ref["launch"], nchunks
            K, k = e.gains()
            assert same(K, ref["K"]) and same(k, ref["k"])          # the resident gains are what came down
            got = taken(out)
    hold_to_oracle(p, dec, got, f"{name} fused={fused}")
    assert not same(ref["K"], reference(name, fused, fp64=True)["K"])      # (and the FP64 payload is another one)


@pytest.mark.parametrize("pipe_copy", ["0", "1", "3"])
def test_upload_follows_the_pipe_copy_switch(pipe_copy, monkeypatch):
    """KPILQR_PIPE_COPY bit 0: the chunk's floats go up by the copy kernel like every other upload (two chunks of panda7: the second
    starts 8 mod 16 bytes into the staging buffer and into the caller's array).  Results only."""
    name, fused = "panda7", True
    p, ref = problem(name), reference(name, fused)
    monkeypatch.setenv("KPILQR_PIPE_COPY", pipe_copy)                         # read when the context is created
    with engine(p, fused) as e:
        inp = setup(e, p)
        pay = pin32(e, columns(name)[1])
        for nchunks in (2, 3):
            out = Outputs(e)
            call3(e, inp, out, nchunks, pay)
            e.sync()
            check(out, ref, what=(pipe_copy, nchunks))


# ---- 2. consecutive calls without a wait, different columns --------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("panda7", True), ("panda5rec", False), ("ragged5", True)])
def test_calls_in_flight_with_different_columns(name, fused):
    p = problem(name)
    refs = [reference(name, fused), reference(name, fused, scale=0.75)]
    assert not same(refs[0]["K"], refs[1]["K"])
    with engine(p, fused) as e:
        inp = setup(e, p)
        pay = [pin32(e, columns(name)[1]), pin32(e, columns(name, 0.75)[1])]
        outs = [Outputs(e) for _ in range(3)]
        call3(e, inp, outs[0], 3, pay[0])
        call3(e, inp, outs[1], 3, pay[1])                        # no sync: the staging ranges are protected by same-stream order
        e.sync()
        check(outs[0], refs[0], what="first")
        check(outs[1], refs[1], what="second")
        call3(e, inp, outs[2], 2, pay[0])                        # another chunk -> stream map
        e.sync()
        check(outs[2], refs[0], what="third")


# ---- 3. with K32 and with the gains of a list ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("panda7", True), ("panda5rec", False), ("pushing3", False), ("ragged5", True)])
def test_combined_with_k32_and_gain_lists(name, fused):
    p, ref = problem(name), reference(name, fused)
    with engine(p, fused) as e:
        inp = setup(e, p)
        c32 = pin32(e, columns(name)[1])
        out = Outputs(e)
        call3(e, inp, out, 3, c32, f32=True)
        e.sync()
        check(out, ref, f32=True, what="K32")
        for i, traj in enumerate(LISTS[p["batch"]]):
            out = Outputs(e)
            call3(e, inp, out, 3, c32, traj=traj, f32=bool(i % 2))
            e.sync()
            check(out, ref, traj=traj, f32=bool(i % 2), what="list")


# ---- 4. without the FP32 columns the new call is kpilqr_iterate_streamed2 -----------------------------------------------------------
def test_null_columns_is_streamed2():
    """fd_kp payload on panda7: whole batch with FP64 K through the raw kpilqr_iterate_streamed2, then K32 of a list through the binding's
    route to it; the same two through kpilqr_iterate_streamed3 with kp_columns32 = NULL on another context"""
    name, fused = "panda7", True
    p = problem(name)
    variants = ((None, False), ([1, 2], True))
    got = {}
    for new in (False, True):
        with engine(p, fused) as e:
            inp = setup(e, p)
            slab = e.fd_kp_slab(*synth.kp_ordered_payload(p))
            for i, (traj, f32) in enumerate(variants):
                out = Outputs(e)
                v = out.view
                kw = dict(fd_kp=slab, K=None if f32 else v["K"], k=v["k"], cost_pred=v["cost_pred"], delta_J=v["delta_J"], status=v["status"],
                          nchunks=3, K32=v["K32"] if f32 else None, gain_traj=traj, **inp)
                if new:
                    e.iterate_streamed3(kp_cols32=None, **kw)
                elif traj is None:
                    io2 = _lib.StreamIO2()                       # kpilqr_iterate_streamed2 itself, also without its options
                    io2.struct_size = C.sizeof(_lib.StreamIO2)
                    io = io2.io
                    io.fd_kp_slab = slab["slab"].ctypes.data; io.entries = slab["entries"]; io.eps = float(p["eps"])
                    for n_ in ("r", "r_x", "r_u", "u_nom", "lam"):
                        setattr(io, n_, inp[n_].ctypes.data)
                    for n_ in OUT:
                        setattr(io, n_, v[n_].ctypes.data)
                    assert e._L.kpilqr_iterate_streamed2(e._h, C.byref(io2), 100, 3) == 0
                else:
                    e.iterate_streamed(**kw)
                e.sync()
                count = None if traj is None else len(traj)
                res = dict((n_, out.rows(n_).copy()) for n_ in ("cost_pred", "delta_J", "status"))
                res["K"] = out.rows("K32" if f32 else "K", count).copy()
                res["k"] = out.rows("k", count).copy()
                out.untouched("K" if f32 else "K32")
                res["launch"] = [e.last_launch(w) for w in ("backward", "forward", "linearise")]
                got[new, i] = res
    for i in range(len(variants)):
        old, new = got[False, i], got[True, i]
        assert old["launch"] == new["launch"], (i, old["launch"], new["launch"])
        for key in OUT:
            assert same(new[key], old[key]), (i, key)
    assert np.all(got[False, 0]["status"] == 0) and np.any(got[False, 0]["K"] != 0)
    assert same(got[False, 1]["K"], cast(got[False, 0]["K"][[1, 2]]))


# ---- 5. the staging buffer grows, and is shared with the explicit call ----------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_staging_growth_and_sharing(fused):
    name, more = "ragged5", (0, 4)                           # then trajectory 0 gets a key-point at every step too: 549 -> 725 entries
    p, p2 = problem(name), problem(name, True, more)
    assert len(columns(name, 1.0, True, more)[1]) > len(columns(name)[1])
    ref, ref2 = reference(name, fused), reference(name, fused, every_step=more)
    ALPHAS = orc.alphas(6)

    def explicit(e, upload):
        upload(e)
        e.iterate(p2["lam"], 100, ALPHAS)
        res = e.results()
        K, k = e.gains()
        return dict(K=K, k=k, cost_pred=res["cost_pred"], delta_J=res["delta_J"], status=res["status"])

    with engine(p2, fused) as e:                             # the explicit step's reference: the FP64 call on the decoded doubles
        setup(e, p2)
        e.upload_residuals(p2["r"], p2["r_x"], p2["r_u"]); e.upload_nominal(p2["u_nom"], None)
        dec2 = columns(name, 1.0, True, more)[2]
        want_explicit = explicit(e, lambda e: e.upload_kp_columns(dict(cols=np.ascontiguousarray(dec2), entries=len(dec2))))
    with engine(p, fused) as e:
        inp = setup(e, p)
        out = Outputs(e)
        call3(e, inp, out, 3, pin32(e, columns(name)[1]))
        e.set_keypoints_rows(p2["kp_rows"])                  # (no sync: the call orders itself behind the chunks)
        c32 = pin32(e, columns(name, 1.0, True, more)[1])
        inp = inputs(e, p2)                                  # (the residuals and controls of the problem with the longer lists)
        out2 = Outputs(e)
        call3(e, inp, out2, 3, c32)                          # the staging buffer has to grow while the first call may be in flight
        e.sync()
        check(out, ref, what="before the growth")
        check(out2, ref2, what="after the growth")
        got = explicit(e, lambda e: e.upload_kp_columns_f32(columns(name, 1.0, True, more)[1]))
        for key in want_explicit:
            assert np.array_equal(got[key], want_explicit[key]), ("explicit upload behind the streamed calls", key)
        out3 = Outputs(e)
        call3(e, inp, out3, 3, c32)
        e.sync()
        check(out3, ref2, what="streamed again behind the explicit upload")


# ---- 6. rejections leave everything alone -------------------------------------------------------------------------------------------
def test_rejected_calls_change_nothing():
    name, fused = "panda7", True
    p, ref = problem(name), reference(name, fused)
    _, c32, dec, _ = columns(name)
    E = len(c32)
    unpinned = np.array(c32.reshape(-1))
    with engine(p, fused) as e:
        inp = setup(e, p)
        pay = pin32(e, c32)
        cols64 = pin64(e, dec)
        slab = e.fd_kp_slab(*synth.kp_ordered_payload(p))
        bad = {
            "outer struct_size + 8": lambda io3: setattr(io3, "struct_size", C.sizeof(_lib.StreamIO3) + 8),
            "outer struct_size - 8": lambda io3: setattr(io3, "struct_size", C.sizeof(_lib.StreamIO3) - 8),
            "inner struct_size + 8": lambda io3: setattr(io3.io2, "struct_size", C.sizeof(_lib.StreamIO2) + 8),
            "inner struct_size - 8": lambda io3: setattr(io3.io2, "struct_size", C.sizeof(_lib.StreamIO2) - 8),
            "unpinned columns": lambda io3: setattr(io3, "kp_columns32", unpinned.ctypes.data),
            "with kp_columns": lambda io3: setattr(io3.io2.io, "kp_columns", cols64["cols"].ctypes.data),
            "with fd_kp_slab": lambda io3: setattr(io3.io2.io, "fd_kp_slab", slab["slab"].ctypes.data),
            "entries + 1": lambda io3: setattr(io3.io2.io, "entries", E + 1),
            "entries - 1": lambda io3: setattr(io3.io2.io, "entries", E - 1),
        }
        for what, spoil in bad.items():
            out = Outputs(e)
            io3 = raw_io3(e, inp, out, pay, E)
            spoil(io3)
            rc = e._L.kpilqr_iterate_streamed3(e._h, C.byref(io3), 100, 3)
            assert rc == _lib.ERR_ARG, (what, rc)
            e.sync()
            out.untouched()
            good = Outputs(e)                                # a valid call behind it
            assert e._L.kpilqr_iterate_streamed3(e._h, C.byref(raw_io3(e, inp, good, pay, E)), 100, 3) == 0, what
            e.sync()
            check(good, ref, what=what)
        assert e._L.kpilqr_iterate_streamed3(e._h, None, 100, 3) == _lib.ERR_ARG
        assert np.array_equal(unpinned, c32.reshape(-1))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_rejected_call_leaves_the_constant_jacobian_mode_alone(fused):
    """A call that carries r_x and is rejected for one of the NEW fields has not ended the constant-Jacobian mode: the iteration behind
    it gives the constant mode's bits and (fused) still reports the rxc form"""
    name = "panda7" if fused else "panda5rec"
    p = problem(name, False)                                 # reaching residuals: one constant r_x, r_u = 0
    _, c32, dec, _ = columns(name, 1.0, False)
    E = len(c32)
    with engine(p, fused) as e:
        inp = setup(e, p, residual_jacobians=False)
        e.upload_residual_jacobians_const(p["rx_const"], None)
        want = Outputs(e)
        v = want.view
        e.iterate_streamed(kp_cols=pin64(e, dec), K=v["K"], k=v["k"], cost_pred=v["cost_pred"], delta_J=v["delta_J"], status=v["status"],
                           nchunks=3, **inp)
        e.sync()
        ref = taken(want)
        launches = [e.last_launch(w) for w in ("backward", "forward")]
        if fused:
            assert all(":rxc" in s for s in launches), launches
        pay = pin32(e, c32)
        rx = e.pinned(p["r_x"].shape); rx[...] = 0.5          # pinned: only the new fields can reject the call
        unpinned = np.array(c32.reshape(-1))
        for spoil in ("outer size", "inner size", "unpinned", "two payloads", "entries"):
            out = Outputs(e)
            io3 = raw_io3(e, inp, out, pay, E)
            io3.io2.io.r_x = rx.ctypes.data
            if spoil == "outer size":
                io3.struct_size -= 8
            elif spoil == "inner size":
                io3.io2.struct_size += 8
            elif spoil == "unpinned":
                io3.kp_columns32 = unpinned.ctypes.data
            elif spoil == "two payloads":
                io3.io2.io.kp_columns = pin64(e, dec)["cols"].ctypes.data
            else:
                io3.io2.io.entries = E + 1
            assert e._L.kpilqr_iterate_streamed3(e._h, C.byref(io3), 100, 3) == _lib.ERR_ARG, spoil
            e.sync()
            out.untouched()
            got = Outputs(e)
            call3(e, inp, got, 3, pay)
            e.sync()
            check(got, ref, what=spoil)
            assert [e.last_launch(w) for w in ("backward", "forward")] == launches, spoil


# ---- 7. the FP64 columns are untouched by a context's FP32 history -------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("ragged5", True), ("panda5rec", False)])
def test_fp64_columns_after_streamed_f32_give_a_fresh_context_s_bits(name, fused):
    p = problem(name)
    cols, c32, _, _ = columns(name)
    want = reference(name, fused, fp64=True)
    with engine(p, fused) as e:
        inp = setup(e, p)
        out = Outputs(e)
        call3(e, inp, out, 3, pin32(e, c32))
        out64 = Outputs(e)
        v = out64.view
        e.iterate_streamed(kp_cols=pin64(e, cols), K=v["K"], k=v["k"], cost_pred=v["cost_pred"], delta_J=v["delta_J"], status=v["status"],
                           nchunks=3, **inp)
        e.sync()
        check(out, reference(name, fused), what="FP32")
        check(out64, want, what="FP64 after FP32")


# ---- 8. special values ---------------------------------------------------------------------------------------------------------------
def test_special_values_arrive_as_the_decoding_rule_says():
    """NaN, +-inf, FP32 subnormals and -0 at unit and at ordinary rows, in the chunks that are NOT the first (entries 4 .. 9 of 12: the
    second and third of three chunks); on a context with step records, A and B show the decoded values at the key-point steps."""
    p = problem("acrobot3")
    dof, n = p["dof"], p["n"]
    _, c32, _, dofs = columns("acrobot3")
    c32 = c32.copy()
    sub = np.float32(1e-40)                                   # an FP32 subnormal
    assert 0 < sub < np.finfo(np.float32).tiny
    specials = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), sub, -sub, np.float32(-0.0)]
    for i, v in enumerate(specials):                          # entry 4 + i: at the unit rows of both kinds, and at ordinary rows of all three
        en = 4 + i
        d = int(dofs[en])
        c32[en, 0, d] = v; c32[en, 1, d + dof] = v
        c32[en, 0, (d + 1) % n] = v; c32[en, 1, d] = v; c32[en, 2, 0] = v
    dec = synth.decode_kp_columns_f32(c32, dofs, dof)
    assert dec[7, 0, int(dofs[7])] == 1.0 and dec[7, 0, (int(dofs[7]) + 1) % n] == np.float64(sub) != 0.0
    assert np.signbit(dec[9, 1, int(dofs[9])]) and dec[9, 1, int(dofs[9])] == 0.0 and dec[9, 0, int(dofs[9])] == 1.0
    offs, times = cf.entry_csr(p)
    assert int(offs[dof]) == 4                                # the first chunk of three ends at entry 4
    with engine(p, False) as e:
        inp = setup(e, p)
        out = Outputs(e)
        call3(e, inp, out, 3, pin32(e, c32))
        e.sync()
        out.rows("K"); out.rows("k")                          # (sentinels; the gains of a trajectory fed NaN are undefined)
        A, B = e.get_AB()
    for b in range(p["batch"]):
        for d in range(dof):
            e0, e1 = int(offs[b * dof + d]), int(offs[b * dof + d + 1])
            ts = times[e0:e1]
            for kind, got in ((0, A[b, ts, d, :]), (1, A[b, ts, d + dof, :])) + (((2, B[b, ts, d, :]),) if d < p["m"] else ()):
                want = dec[e0:e1, kind]
                assert np.array_equal(got, want, equal_nan=True), (b, d, kind)
                ok = ~np.isnan(want)
                assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok])), (b, d, kind)       # -0 stays -0 off the unit rows
