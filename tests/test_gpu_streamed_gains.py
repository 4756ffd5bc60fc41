"""GPU tests of kpilqr_iterate_streamed2 (csrc/gains.hip: k_gains_out): the chunk pipeline bringing K down as FP32 and the gains of a
list of trajectories alone, gathered and stored straight into the caller's pinned buffers.

Shapes (the smallest at which the indexing can still go wrong; every sweep form accepts these horizons, so none was replaced):
  panda_reaching  T = 17, batch 7, fused    1666 elements of K per trajectory (2 mod 4: a float row is 8- but not 16-byte aligned),
                                            k rows of 119 elements (odd: every second row is off 16-byte alignment)
  acrobot         T = 5,  batch 3, fused    20 elements of K, k rows of 5
  panda_reaching  T = 17, batch 5, on a context with step records
  panda_pushing   T = 17, batch 3, a tiled shape (2380 elements of K, k rows of 119)
Every output lies inside a larger pinned allocation between 64 sentinel elements, and is sized for the WHOLE batch also when a list
is given: the rows behind the listed ones have to stay sentinel.  The reference of a shape is ONE streamed FP64 run through
kpilqr_iterate_streamed on a fresh context, made once and shared; the reference of the conversion is numpy's float64 -> float32 cast,
which tests/test_gpu_gains_f32.py checks on the values whose rounding it knows."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from trajoptkp_amd import Engine, _lib, synth

pytestmark = pytest.mark.gpu

PAD = 64
SENT = {np.dtype(np.float64): -7.25, np.dtype(np.float32): np.float32(-7.25), np.dtype(np.int32): np.int32(-77)}
SHAPES = {      # name: (task, T, batch, fused)
    "panda7": ("panda_reaching", 17, 7, True),
    "acrobot3": ("acrobot", 5, 3, True),
    "panda5rec": ("panda_reaching", 17, 5, False),
    "pushing3": ("panda_pushing", 17, 3, False),
}
# Three chunks cut a batch of 7 into [0,2), [2,4), [4,7), one of 5 into [0,1), [1,3), [3,5), one of 3 into single trajectories.
# whole batch | no gains | first | last | straddling a chunk boundary | scattered (with an adjacent run where the batch has room) |
# the last chunk only | everybody
LISTS = {
    7: [None, [], [0], [6], [1, 2], [0, 1, 3, 6], [4, 5, 6], [0, 1, 2, 3, 4, 5, 6]],
    5: [None, [], [0], [4], [0, 1], [0, 1, 3], [3, 4], [0, 1, 2, 3, 4]],
    3: [None, [], [0], [2], [0, 1], [0, 2], [0, 1, 2]],           # (the last chunk only is [2])
}


def cast(K):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(K, np.float64).astype(np.float32)


def same(got, want):
    """bit for bit"""
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(u), want.view(u))


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / np.max(np.abs(b)))


@functools.lru_cache(maxsize=None)
def problem(name, weight_scale=1.0, dense=True):
    task, T, batch, _ = SHAPES[name]
    p = synth.make_problem(task=task, T=T, batch=batch, min_N=5, dense_residuals=dense)
    if weight_scale != 1.0:
        p["w_run"] = p["w_run"] * weight_scale; p["w_term"] = p["w_term"] * weight_scale
    p["payload"] = synth.kp_ordered_payload(p)
    return p


def engine(name, p):
    return Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=SHAPES[name][3])


def setup(e, p, residual_jacobians=True):
    """Everything a streamed iteration needs beside its own arguments; returns those: the pinned key-point ordered payload and inputs."""
    e.set_keypoints_rows(p["kp_rows"])
    e.upload_residuals(None, None, None, p["w_run"], p["w_term"])
    e.upload_nominal(None, p["ctrl_lim"])
    e.forward_linear(orc.alphas(6), fetch=False)                  # (the alphas)
    inp = dict(fd_kp=e.fd_kp_slab(*p["payload"]), eps=p["eps"])
    for name in ("r", "r_x", "r_u", "u_nom") if residual_jacobians else ("r", "u_nom"):
        inp[name] = e.pinned(p[name].shape); inp[name][...] = p[name]
    inp["lam"] = e.pinned(p["batch"]); inp["lam"][:] = p["lam"]
    return inp


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


def call(e, inp, out, nchunks, traj=None, f32=False, want_k=True, payload=True):
    """Engine.iterate_streamed into `out` (no wait): K as FP64 or FP32, of the whole batch or of `traj`"""
    kw = dict(inp) if payload else dict(lam=inp["lam"])
    v = out.view
    e.iterate_streamed(K=None if f32 else v["K"], k=v["k"] if want_k else None, cost_pred=v["cost_pred"], delta_J=v["delta_J"],
                       status=v["status"], nchunks=nchunks, K32=v["K32"] if f32 else None, gain_traj=traj, **kw)


def check(out, ref, traj=None, f32=False, want_k=True):
    """after sync(): the outputs of call() against the reference of the shape"""
    rows = np.arange(out.B) if traj is None else np.array(traj, np.int64)
    if f32:
        assert same(out.rows("K32", len(rows)), cast(ref["K"][rows])), (traj, "K32 is not the cast of K")
        out.untouched("K")
    else:
        assert same(out.rows("K", len(rows)), ref["K"][rows]), (traj, "K")
        out.untouched("K32")
    if want_k:
        assert same(out.rows("k", len(rows)), ref["k"][rows]), (traj, "k")
    else:
        out.untouched("k")
    for name in ("cost_pred", "delta_J", "status"):               # whole-batch outputs whatever the list says
        assert same(out.rows(name), ref[name]), (traj, name)


def raw_io2(e, inp, out, K=True, k=True):
    """kpilqr_stream_io2 with the standard inputs and outputs; the caller changes fields before it calls"""
    io2 = _lib.StreamIO2()
    io2.struct_size = C.sizeof(_lib.StreamIO2)
    io = io2.io
    io.fd_kp_slab = inp["fd_kp"]["slab"].ctypes.data; io.entries = inp["fd_kp"]["entries"]; io.eps = float(inp["eps"])
    for name in ("r", "r_x", "r_u", "u_nom", "lam"):
        if name in inp:
            setattr(io, name, inp[name].ctypes.data)
    for name in ("K", "k", "cost_pred", "delta_J", "status"):
        if (name != "K" or K) and (name != "k" or k):
            setattr(io, name, out.view[name].ctypes.data)
    return io2


_REF = {}


def reference(name):
    """K, k, cost_pred, delta_J, status and the three launch descriptions of ONE kpilqr_iterate_streamed (three chunks) on a fresh context"""
    if name not in _REF:
        p = problem(name)
        with engine(name, p) as e:
            inp = setup(e, p)
            out = Outputs(e)
            call(e, inp, out, 3)
            e.sync()
            ref = dict((n, out.rows(n).copy()) for n in ("K", "k", "cost_pred", "delta_J", "status"))
            out.untouched("K32")
            ref["launch"] = [e.last_launch(w) for w in ("backward", "forward", "linearise")]
            K, k = e.gains()
            assert same(K, ref["K"]) and same(k, ref["k"])          # the resident gains are what came down
        assert np.all(ref["status"] == 0) and np.all(np.isfinite(ref["K"]))
        _REF[name] = ref
    return _REF[name]


def chunk_counts(name):
    return sorted({1, 3, SHAPES[name][2]})


# ---- 1. without the options the new call is the old one ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_without_options_the_new_call_is_the_old_one(name):
    p, ref = problem(name), reference(name)
    for nchunks in chunk_counts(name):
        got = []
        for new in (False, True):
            with engine(name, p) as e:
                inp = setup(e, p)
                out = Outputs(e)
                if new:
                    assert e._L.kpilqr_iterate_streamed2(e._h, C.byref(raw_io2(e, inp, out)), 100, nchunks) == 0
                else:
                    call(e, inp, out, nchunks)
                e.sync()
                got.append(dict((n, out.rows(n).copy()) for n in ("K", "k", "cost_pred", "delta_J", "status")))
                out.untouched("K32")
                got[-1]["launch"] = [e.last_launch(w) for w in ("backward", "forward", "linearise")]
        for n in ("K", "k", "cost_pred", "delta_J", "status"):
            assert same(got[1][n], got[0][n]), (nchunks, n)
            assert same(got[0][n], ref[n]), (nchunks, n, "the chunk count changed a result")
        assert got[1]["launch"] == got[0]["launch"], (nchunks, got[0]["launch"], got[1]["launch"])


# ---- 2. FP32 and lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nchunks", [(n, c) for n in SHAPES for c in chunk_counts(n)])
def test_fp32_and_lists(name, nchunks):
    p, ref = problem(name), reference(name)
    with engine(name, p) as e:
        inp = setup(e, p)
        first = True
        for i, traj in enumerate(LISTS[p["batch"]]):
            for f32 in (False, True):
                if traj is None and not f32:
                    continue                                            # (the old call: test 1)
                want_k = not (f32 and i % 2)                            # K32 of every second list comes down without k
                out = Outputs(e)
                call(e, inp, out, nchunks, traj=traj, f32=f32, want_k=want_k, payload=first or i % 3 == 0)      # (also on the resident payload)
                first = False
                e.sync()
                check(out, ref, traj=traj, f32=f32, want_k=want_k)
                K, k = e.gains()
                assert same(K, ref["K"]) and same(k, ref["k"]), (traj, f32, "the resident gains changed")
        assert [e.last_launch(w) for w in ("backward", "forward")] == ref["launch"][:2]


def test_k32_against_the_oracle():
    """K32 within 1e-6 (relative to max |K|) of the CPU oracle: 2^-24 of rounding on top of the 1e-9 parity of K"""
    from oracle import pipeline
    p = problem("panda7")
    with engine("panda7", p) as e:
        inp = setup(e, p)
        out = Outputs(e)
        call(e, inp, out, 3, f32=True)
        e.sync()
        K32 = out.rows("K32")
        assert np.all(out.rows("status") == 0)
    for b in range(p["batch"]):
        o = pipeline.run_trajectory(p, b)
        err = relerr(K32[b], o["K"])
        print(f"trajectory {b}: K32 against the oracle's K: {err:.3e} relative")
        assert o["status"] == 0 and err < 1e-6, (b, err)


# ---- 3. subnormals come out of THIS kernel ------------------------------------------------------------------------------------------
def test_subnormals_are_produced_not_flushed():
    """Weights times 1e-41: the gains lie in the FP32 subnormal range.  Checked on the CPU oracle for this problem: status 0 for all
    seven trajectories; for trajectories 0, 3 and 4 all 1666 elements of K lie between 1.6e-45 and 1.4e-41, inside (2^-149, 2^-126),
    and none casts to zero (the other four have a few elements below 2^-149 = 1.4e-45, one of which, in trajectory 6, rounds to zero;
    at 1e-42 more do).  The preconditions are asserted on those three trajectories, the bits on all seven.  A kernel that flushed
    would return zeros."""
    p = problem("panda7", 1e-41)
    sub = [0, 3, 4]
    with engine("panda7", p) as e:
        inp = setup(e, p)
        out = Outputs(e)
        call(e, inp, out, 3)
        e.sync()
        K = out.rows("K").copy()
        assert np.all(out.rows("status") == 0)
        assert np.all(np.abs(K[sub]) > 2.0 ** -149) and np.all(np.abs(K[sub]) < 2.0 ** -126), (np.min(np.abs(K[sub])), np.max(np.abs(K[sub])))
        assert np.all(np.abs(K) < 2.0 ** -126)
        want = cast(K)
        assert not np.any(want[sub] == 0)
        for traj in (None, sub, [0, 1, 3, 6]):
            out = Outputs(e)
            call(e, inp, out, 3, traj=traj, f32=True)
            e.sync()
            rows = np.arange(7) if traj is None else np.array(traj)
            got = out.rows("K32", len(rows))
            assert not np.any(got[np.isin(rows, sub)] == 0), "flushed"
            assert same(got, want[rows]), traj


# ---- 4. consecutive calls without a wait -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda7", "panda5rec"])
def test_three_calls_in_flight(name):
    """L, L again (no upload of the list, no wait), then another list with K32 (joins the pipeline first): three sets of outputs, one sync"""
    p, ref = problem(name), reference(name)
    B = p["batch"]
    L1, L2 = LISTS[B][5], [1, 2, B - 1]
    with engine(name, p) as e:
        inp = setup(e, p)
        outs = [Outputs(e) for _ in range(3)]
        call(e, inp, outs[0], 3, traj=L1)
        call(e, inp, outs[1], 3, traj=list(L1))
        call(e, inp, outs[2], 3, traj=L2, f32=True)
        e.sync()
        check(outs[0], ref, traj=L1)
        check(outs[1], ref, traj=L1)
        check(outs[2], ref, traj=L2, f32=True)


# ---- 5. rejections change nothing ---------------------------------------------------------------------------------------------------
def test_rejected_calls_change_nothing():
    name = "panda7"
    p, ref = problem(name), reference(name)
    B = p["batch"]
    unpinned = np.zeros(B * p["T"] * p["n"] * p["m"], np.float32)
    keep = []

    def lst(io2, values, count=None):
        a = np.array(values, np.int32); keep.append(a)
        io2.gain_traj = a.ctypes.data; io2.gain_count = len(a) if count is None else count
        io2.K32 = 0

    def k32(io2, ptr, keepK=False):
        io2.K32 = ptr
        if not keepK:
            io2.io.K = None

    with engine(name, p) as e:
        inp = setup(e, p)
        bad = {
            "io.K and K32": lambda io2, out: k32(io2, out.view["K32"].ctypes.data, keepK=True),
            "unpinned K32": lambda io2, out: k32(io2, unpinned.ctypes.data),
            "K32 at 4 mod 8": lambda io2, out: k32(io2, out.view["K32"].ctypes.data + 4),
            "[2,1]": lambda io2, out: lst(io2, [2, 1]),
            "[1,1]": lambda io2, out: lst(io2, [1, 1]),
            "[0,batch]": lambda io2, out: lst(io2, [0, B]),
            "[-1,0]": lambda io2, out: lst(io2, [-1, 0]),
            "gain_count -1": lambda io2, out: lst(io2, [0], count=-1),
            "gain_count 1, NULL list": lambda io2, out: (setattr(io2, "gain_count", 1), setattr(io2, "gain_traj", None)),
            "struct_size + 8": lambda io2, out: setattr(io2, "struct_size", C.sizeof(_lib.StreamIO2) + 8),
            "struct_size - 8": lambda io2, out: setattr(io2, "struct_size", C.sizeof(_lib.StreamIO2) - 8),
        }
        for what, spoil in bad.items():
            out = Outputs(e)
            assert out.view["K32"].ctypes.data % 8 == 0                          # (so that + 4 is 4 mod 8)
            io2 = raw_io2(e, inp, out)
            spoil(io2, out)
            rc = e._L.kpilqr_iterate_streamed2(e._h, C.byref(io2), 100, 3)
            assert rc == _lib.ERR_ARG, (what, rc)
            e.sync()
            out.untouched()
            assert np.all(unpinned == 0), what
            good = Outputs(e)                                                   # a valid call behind it: the results of test 1
            assert e._L.kpilqr_iterate_streamed2(e._h, C.byref(raw_io2(e, inp, good)), 100, 3) == 0, what
            e.sync()
            check(good, ref)
        assert e._L.kpilqr_iterate_streamed2(e._h, None, 100, 3) == _lib.ERR_ARG


@pytest.mark.parametrize("fused", [True, False])
def test_rejected_call_leaves_the_constant_jacobian_mode_alone(fused):
    """A call that carries r_x and is rejected for one of the NEW fields has not ended the constant-Jacobian mode: the iteration
    behind it gives the constant mode's bytes (had the mode been left, the sweeps would read an r_x buffer nobody filled)."""
    name = "panda7" if fused else "panda5rec"
    p = problem(name, 1.0, False)                                            # reaching residuals: one constant r_x, r_u = 0
    with engine(name, p) as e:
        inp = setup(e, p, residual_jacobians=False)
        e.upload_residual_jacobians_const(p["rx_const"], None)
        want = Outputs(e)
        call(e, inp, want, 3)
        e.sync()
        launches = [e.last_launch(w) for w in ("backward", "forward")]
        rx = e.pinned(p["r_x"].shape); rx[...] = 0.5                          # pinned: only the new fields can reject the call
        for spoil in ("list", "K32", "size"):
            out = Outputs(e)
            io2 = raw_io2(e, inp, out)
            io2.io.r_x = rx.ctypes.data
            tr = np.array([1, 1], np.int32)
            if spoil == "list":
                io2.gain_traj = tr.ctypes.data; io2.gain_count = 2
            elif spoil == "K32":
                io2.K32 = out.view["K32"].ctypes.data + 4; io2.io.K = None
            else:
                io2.struct_size -= 8
            assert e._L.kpilqr_iterate_streamed2(e._h, C.byref(io2), 100, 3) == _lib.ERR_ARG, spoil
            e.sync()
            out.untouched()
            got = Outputs(e)
            call(e, inp, got, 3, traj=[0, 2], f32=True, payload=False)
            e.sync()
            ref = dict((n, want.rows(n)) for n in ("K", "k", "cost_pred", "delta_J", "status"))
            check(got, ref, traj=[0, 2], f32=True)
            assert [e.last_launch(w) for w in ("backward", "forward")] == launches


# ---- 6. KPILQR_PIPE_COPY ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe_copy", ["0", "1", "3"])
def test_pipe_copy_switch_does_not_reach_the_gather(pipe_copy, monkeypatch):
    """The K32 and list downloads take the gather kernel whatever the switch says; the old entry point still follows it.  Results only."""
    name = "panda7"
    p, ref = problem(name), reference(name)
    monkeypatch.setenv("KPILQR_PIPE_COPY", pipe_copy)                         # read when the context is created
    with engine(name, p) as e:
        inp = setup(e, p)
        for traj, f32 in ((None, False), (None, True), ([0, 1, 3, 6], True), ([0, 1, 3, 6], False), ([1, 2], True)):
            out = Outputs(e)
            call(e, inp, out, 3, traj=traj, f32=f32)
            e.sync()
            check(out, ref, traj=traj, f32=f32)
