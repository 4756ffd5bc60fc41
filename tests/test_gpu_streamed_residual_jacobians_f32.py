"""GPU tests of kpilqr_iterate_streamed6 (csrc/residuals_f32.hip: k_widen_jacobians): the chunk pipeline taking the per-step residual
Jacobians r_x / r_u as FP32 -- per chunk one upload per array into the chunk's region of the context's staging buffer (or, with
KPILQR_PIPE_COPY bit 0, none: the kernel reads the caller's pinned floats) and ONE launch that widens both arrays into the FP64 buffers.

The yardstick is never the code under test: every case runs the same calls on a second, fresh context of the same flags through
kpilqr_iterate_streamed5 (kpilqr_iterate_streamed4 where only upload_traj is given) fed the numpy-widened doubles, astype(float64) of
the floats, as FP64 io.r_x / io.r_u with the same nchunks.  K, k, cost_pred, delta_J, status must be equal bit for bit, so must the
kpilqr_last_launch strings and -- read last, fetching KPILQR_BUF_R_U ends :ru0 -- the r_x / r_u device buffers.  K and k of the whole
call on acrobot5 and panda3 are also held to the C oracle run on the widened Jacobians at the suite's 1e-9.

Shapes (the smallest at which the chunk and parity indexing can go wrong; dense residuals, min_N = 5):
  acrobot5   acrobot        T = 36, batch 5, fused     r_u has 37 * 5 * 1 = 185 elements per trajectory, odd: the element path; with
                                                       three chunks (trajectories 0 | 1-2 | 3-4) chunk 1's slice of r_u32 starts on an
                                                       odd float.  nchunks 0 (= 3), 2 and 5
  panda3     panda_reaching T = 37, batch 3, fused and on a context with step records; r_x is 7448 elements per trajectory: several
                                                       slices of pairs
  pushing3   panda_pushing  T = 17, batch 3, the tiled family
  m_gt_dof   (dof, m, nr) = (3, 5, 3), T = 33, batch 2: nchunks is clipped to the batch
The FD payload is resident (job lists, an ordinary upload before the first streamed call), so the streamed calls carry the Jacobians,
lambda and the outputs; the everything-at-once case brings encoded FP32 columns.  Every output lies inside a larger pinned allocation
between 64 sentinel elements (Outputs of tests/test_gpu_streamed_columns_f32.py).  A library without the symbol fails these tests."""
import ctypes as C
import functools

import numpy as np
import pytest

import _residual_jacobians_f32 as rj
import _streamed_subset as ss
from oracle import oracle as orc
from oracle import pipeline
from test_gpu_streamed_columns_f32 import Outputs, TIGHT, cast as cast_gains, relerr, same
from trajoptkp_amd import Engine, _lib, synth
from trajoptkp_amd.engine import KpilqrError

pytestmark = pytest.mark.gpu

OUT = ("K", "k", "cost_pred", "delta_J", "status")
SHAPES = {      # name: make_problem's arguments
    "acrobot5": dict(task="acrobot", T=36, batch=5, min_N=5, config_id=1),
    "panda3": dict(task="panda_reaching", T=37, batch=3, min_N=5, config_id=2),
    "pushing3": dict(task="panda_pushing", T=17, batch=3, min_N=5, config_id=3),
    "m_gt_dof": dict(task=synth.shape_task(3, 5, 3), T=33, batch=2, min_N=4, config_id=4),
}
CONTEXTS = [("acrobot5", True), ("panda3", True), ("panda3", False), ("pushing3", False), ("m_gt_dof", False)]      # (m > dof has no fused form)
IDS = [f"{n}-{'fused' if f else 'records'}" for n, f in CONTEXTS]
NCHUNKS = {"acrobot5": (0, 2, 5), "panda3": (0, 2), "pushing3": (0,), "m_gt_dof": (0,)}
# upload_traj with three chunks: the first trajectory | the last | a pair straddling a chunk boundary | nobody | one chunk without a listed trajectory
UPLOAD_LISTS = {"acrobot5": [[0], [4], [2, 3], [], [0, 4]], "panda3": [[0], [2], [0, 1], [], [0, 2]]}
PIPE_COPY = [None, "3"]
PIPE_IDS = ["sdma", "pipe_copy3"]


# ---- problems, floats and their twins ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(name, seed=None, dense=True):
    kw = dict(SHAPES[name])
    if seed is not None:
        kw["config_id"] = seed
    return synth.make_problem(dense_residuals=dense, **kw)


@functools.lru_cache(maxsize=None)
def floats(name, seed=None):
    """(r_x32, r_u32) of a shape -- seed: from another draw of the problem -- and, asserted, that their widening is not the FP64 data"""
    p = problem(name, seed)
    x32, u32 = synth.residual_jacobians_f32(p)
    q = rj.decoded_twin(p)
    assert np.array_equal(rj.decode(x32), q["r_x"]) and np.array_equal(rj.decode(u32), q["r_u"])
    assert np.count_nonzero(q["r_x"] != p["r_x"]) > p["r_x"].size // 4          # the transport rounds: this is not FP64 in disguise
    assert np.count_nonzero(q["r_x"] != p["r_x"]) + np.count_nonzero(q["r_u"] != p["r_u"]) > (p["r_x"].size + p["r_u"].size) // 4
    x32.setflags(write=False); u32.setflags(write=False)
    return x32, u32


def test_shapes_are_the_ones_the_chunks_and_parities_are_cut_by():
    p = problem("acrobot5")
    per_u, per_x = int(np.prod(p["r_u"].shape[1:])), int(np.prod(p["r_x"].shape[1:]))
    assert (per_u, per_x % 2) == (185, 0) and p["batch"] == 5
    assert (1 * per_u) % 2 == 1                                  # chunk 1 of three (trajectories 1-2) starts on an odd float of r_u32
    assert int(np.prod(problem("panda3")["r_x"].shape[1:])) == 7448 > 2 * 2048      # several slices of 2048 pairs
    q = problem("m_gt_dof")
    assert q["m"] > q["dof"] and q["batch"] == 2


# ---- contexts, calls, what is compared --------------------------------------------------------------------------------------------------
def engine(p, fused):
    return Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=fused)


def base(e, p):
    """Everything but the residual Jacobians, by ordinary calls: key-points, the FD payload (job lists), r and the weights, the nominal
    controls and their limits, the alphas"""
    e.set_keypoints_rows(p["kp_rows"])
    e.upload_fd(p["job_b"], p["job_t"], p["job_col"], p["job_mode"], p["xplus"], p["xminus"], job_nom=p["job_nom"], xnom=p["xnom"], eps=p["eps"])
    e.upload_residuals(p["r"], None, None, p["w_run"], p["w_term"])
    e.upload_nominal(p["u_nom"], p["ctrl_lim"])
    e.forward_linear(orc.alphas(6), fetch=False)


def pin(e, a):
    """a pinned copy (an empty array keeps a valid address)"""
    a = np.ascontiguousarray(a)
    b = e.pinned(max(a.size, 1), a.dtype)
    b[:a.size] = a.reshape(-1)
    return b[:a.size]


def call(e, p, new, nchunks=3, r_x=None, r_u=None, upload=None, sweep=None, gain=None, K32=False, lam=None, kp_cols32=None):
    """One streamed call, no wait -> its Outputs.  r_x / r_u are WHOLE-BATCH arrays (with upload_traj the listed rows are taken from
    them): float32 ones cross as FP32 through the new call and as their widened doubles through the twin; float64 ones are FP64 on
    both.  new: kpilqr_iterate_streamed6; else kpilqr_iterate_streamed5, or kpilqr_iterate_streamed4 for upload_traj alone."""
    out = Outputs(e)
    v = out.view
    kw = dict(K=None if K32 else v["K"], k=v["k"], cost_pred=v["cost_pred"], delta_J=v["delta_J"], status=v["status"], nchunks=nchunks,
              K32=v["K32"] if K32 else None, gain_traj=gain, eps=p["eps"], kp_cols32=kp_cols32)
    rows = None if upload is None else np.asarray(upload, np.int64)
    for key, a in (("r_x", r_x), ("r_u", r_u)):
        if a is None:
            continue
        a = a if rows is None else a[rows]
        if a.dtype == np.float32 and new:
            kw[key + "32"] = pin(e, a).reshape(a.shape)
        else:
            kw[key] = pin(e, a.astype(np.float64)).reshape(a.shape)
    count = p["batch"] if sweep is None else len(sweep)
    kw["lam"] = pin(e, np.full(count, float(p["lam"])) if lam is None else np.asarray(lam, np.float64))
    out.keep = kw                                               # (the pinned inputs live as long as the outputs)
    if new:
        e.iterate_streamed6(upload_traj=upload, sweep_traj=sweep, **kw)
    elif sweep is None and upload is not None:
        e.iterate_streamed4(upload_traj=upload, **kw)
    else:
        e.iterate_streamed5(upload_traj=upload, sweep_traj=sweep, **kw)
    return out


def launches(e):
    return [e.last_launch(w) for w in ("backward", "forward", "linearise")]


def grab(e, out, sweep=None, gain=None, K32=False):
    """after sync(): the rows a call brought down (sentinels everywhere else, asserted) and the launch strings"""
    ns, ng = None if sweep is None else len(sweep), None if gain is None else len(gain)
    res = dict((key, out.rows(key, ns).copy()) for key in ("cost_pred", "delta_J", "status"))
    res["K"] = out.rows("K32" if K32 else "K", ng).copy()
    out.untouched("K" if K32 else "K32")
    res["k"] = out.rows("k", ng).copy()
    res["launch"] = launches(e)
    return res


def resident(e):
    """the device-resident outputs of the sweeps, whole batch"""
    K, k = e.gains()
    return dict(K=K, k=k, **e.results())


def buffers(e, p, which=("r_x", "r_u")):
    """The r_x / r_u device buffers.  LAST on a context: kpilqr_device_ptr hands out a writable pointer, and fetching r_u ends :ru0"""
    import torch
    e.sync()
    got = {}
    for key in which:
        buf = _lib.BUF_R_X if key == "r_x" else _lib.BUF_R_U
        got[key] = torch.as_tensor(e.device_array(buf, p[key].shape), device=f"cuda:{e.device}").cpu().numpy().copy()
    return got


def equal(got, want, what):
    assert set(got) == set(want), what
    for key in want:
        if key == "launch":
            assert got[key] == want[key], (what, got[key], want[key])
        else:
            assert same(np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])), (what, key)


def both(p, fused, scenario, read=("r_x", "r_u"), prepare=base):
    """scenario(e, new) -> {label: results} on two fresh contexts: the twin (new = False) and the new call; everything is compared, then
    the r_x / r_u buffers.  -> (the twin's results, the new call's, the new call's buffers)"""
    got = []
    for new in (False, True):
        with engine(p, fused) as e:
            prepare(e, p)
            res = scenario(e, new)
            got.append((res, buffers(e, p, read)))
    (want, want_buf), (res, buf) = got
    assert set(res) == set(want)
    for label in want:
        equal(res[label], want[label], label)
    for key in want_buf:
        assert same(buf[key], want_buf[key]), (key, "device buffer")
    return want, res, buf


def widened(a32):
    return np.asarray(a32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def oracle_gains(name):
    """K, k of the C oracle's pipeline on the widened Jacobians"""
    q = rj.decoded_twin(problem(name))
    return [pipeline.run_trajectory(q, b) for b in range(q["batch"])]


def hold_to_oracle(name, got, what):
    for b, o in enumerate(oracle_gains(name)):
        assert o["status"] == 0 and got["status"][b] == 0, (what, b)
        eK, ek = relerr(got["K"][b], o["K"]), relerr(got["k"][b], o["k"])
        print(f"{what} b={b}: K {eK:.2e} k {ek:.2e} against the oracle on the widened Jacobians")
        assert eK < TIGHT and ek < TIGHT, (what, b, eK, ek)


def set_pipe_copy(monkeypatch, value):
    monkeypatch.delenv("KPILQR_PIPE_COPY", raising=False)           # read when a context is created
    if value is not None:
        monkeypatch.setenv("KPILQR_PIPE_COPY", value)


# ---- 1. whole batch, both arrays -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe_copy", PIPE_COPY, ids=PIPE_IDS)
@pytest.mark.parametrize("name,fused", CONTEXTS, ids=IDS)
def test_whole_batch_equals_its_fp64_twin(name, fused, pipe_copy, monkeypatch):
    set_pipe_copy(monkeypatch, pipe_copy)
    p = problem(name)
    x32, u32 = floats(name)

    def scenario(e, new):
        res = {}
        for nchunks in NCHUNKS[name]:
            out = call(e, p, new, nchunks, x32, u32)
            e.sync()
            res[nchunks] = grab(e, out)
            assert all(same(a, res[nchunks][key]) for key, a in resident(e).items()), nchunks      # the resident outputs are what came down
        return res

    want, got, buf = both(p, fused, scenario)
    assert same(buf["r_x"], widened(x32)) and same(buf["r_u"], widened(u32))
    for nchunks, r in want.items():
        assert np.all(r["status"] == 0) and np.any(r["K"] != 0) and np.all(np.isfinite(r["K"])), nchunks
        for s in got[nchunks]["launch"][:2]:
            assert s and ":rxc" not in s and ":ru0" not in s, s
    if name in ("acrobot5", "panda3"):
        hold_to_oracle(name, got[NCHUNKS[name][0]], f"{name} fused={fused}")


def test_the_fp64_jacobians_give_other_bits():
    """(what the twin is compared with is not the FP64 problem again)"""
    name, fused = "acrobot5", True
    p = problem(name)
    x32, u32 = floats(name)
    res = []
    for rx, ru in ((x32, u32), (p["r_x"], p["r_u"])):
        with engine(p, fused) as e:
            base(e, p)
            out = call(e, p, True, 3, rx, ru)
            e.sync()
            res.append(grab(e, out))
    assert not same(res[0]["K"], res[1]["K"]) and res[0]["launch"] == res[1]["launch"]


# ---- 2. r_x32 alone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe_copy", PIPE_COPY, ids=PIPE_IDS)
def test_r_x32_alone_keeps_the_context_without_control_residuals(pipe_copy, monkeypatch):
    set_pipe_copy(monkeypatch, pipe_copy)
    name, fused = "acrobot5", True
    p = problem(name)
    x32, _ = floats(name)

    def scenario(e, new):
        out = call(e, p, new, 3, x32, None)
        e.sync()
        return {"r_x32 alone": grab(e, out)}

    want, got, buf = both(p, fused, scenario)
    assert same(buf["r_x"], widened(x32))
    assert not np.any(buf["r_u"]) and not np.any(np.signbit(buf["r_u"]))          # exactly zero
    for r in (want, got):
        back, fwd, _ = r["r_x32 alone"]["launch"]
        assert ":ru0" in back and ":ru0" in fwd and ":rxc" not in back, r["r_x32 alone"]["launch"]


# ---- 3. mixed transports ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("acrobot5", True), ("panda3", False)], ids=["acrobot5-fused", "panda3-records"])
def test_one_array_as_fp32_beside_the_other_as_fp64(name, fused):
    p = problem(name)
    x32, u32 = floats(name)

    def scenario(e, new):
        res = {}
        for label, rx, ru in (("r_x32 + r_u", x32, p["r_u"]), ("r_x + r_u32", p["r_x"], u32)):
            out = call(e, p, new, 3, rx, ru)
            e.sync()
            res[label] = grab(e, out)
        return res

    want, got, buf = both(p, fused, scenario)
    assert same(buf["r_x"], np.asarray(p["r_x"], np.float64)) and same(buf["r_u"], widened(u32))
    assert not same(want["r_x32 + r_u"]["K"], want["r_x + r_u32"]["K"])
    assert np.all(want["r_x + r_u32"]["status"] == 0)


# ---- 4. upload_traj --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe_copy", PIPE_COPY, ids=PIPE_IDS)
@pytest.mark.parametrize("name,fused", [("acrobot5", True), ("panda3", True), ("panda3", False)], ids=["acrobot5-fused", "panda3-fused", "panda3-records"])
def test_listed_rows_arrive_and_nobody_else_s_are_touched(name, fused, pipe_copy, monkeypatch):
    """Before every listed call a whole FP64 upload of ANOTHER draw fills r_x / r_u: the unlisted rows keep those bits, the listed rows
    hold the widened floats.  The twin is kpilqr_iterate_streamed4 with the compact widened FP64 rows."""
    set_pipe_copy(monkeypatch, pipe_copy)
    p, other = problem(name), problem(name, 11)
    x32, u32 = floats(name)
    assert not np.array_equal(other["r_x"], p["r_x"]) and not np.array_equal(other["r_u"], p["r_u"])
    seen = {}

    def scenario(e, new):
        res = {}
        for traj in UPLOAD_LISTS[name]:
            e.upload_residuals(None, other["r_x"], other["r_u"])        # (an ordinary call: it orders itself behind the pipeline)
            out = call(e, p, new, 3, x32, u32, upload=traj)
            e.sync()
            res[str(traj)] = grab(e, out)
            if new:
                seen[str(traj)] = buffers(e, p)
            else:
                buffers(e, p)                                           # (the same calls on both contexts)
        return res

    want, got, _ = both(p, fused, scenario)
    for traj in UPLOAD_LISTS[name]:
        kept = [b for b in range(p["batch"]) if b not in traj]
        for key, a32 in (("r_x", x32), ("r_u", u32)):
            buf = seen[str(traj)][key]
            assert same(buf[traj], widened(a32)[traj]), (traj, key, "the listed rows")
            assert same(buf[kept], np.asarray(other[key], np.float64)[kept]), (traj, key, "an unlisted trajectory's rows were written")
        assert np.all(want[str(traj)]["status"] == 0), traj
    assert not same(want["[0]"]["K"], want["[]"]["K"])


# ---- 5. sweep_traj with an upload_traj inside it -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused,sweep,upload", [("acrobot5", True, [0, 1, 3], [1]), ("panda3", False, [0, 2], [2]), ("panda3", True, [0, 1, 2], [0, 2])],
                         ids=["acrobot5-fused", "panda3-records", "panda3-fused"])
def test_listed_sweeps_with_listed_uploads(name, fused, sweep, upload):
    """Three chunks; on acrobot5 chunks 0 and 2, on panda3 (records) chunk 0 sweep a listed trajectory and upload nothing.  The twin is
    kpilqr_iterate_streamed5; lambda, cost_pred, delta_J and status are compact."""
    p = problem(name)
    x32, u32 = floats(name)
    y32, v32 = floats(name, 11)
    lam = float(p["lam"]) * (1.5 + 0.25 * np.arange(len(sweep)))
    snap = {}

    def scenario(e, new):
        res = {}
        out = call(e, p, new, 3, x32, u32)
        e.sync()
        res["whole"] = grab(e, out)
        snap[new] = resident(e)
        out = call(e, p, new, 3, y32, v32, upload=upload, sweep=sweep, lam=lam)
        e.sync()
        res["listed"] = grab(e, out, sweep=sweep)
        res["resident"] = resident(e)
        return res

    want, got, buf = both(p, fused, scenario)
    kept = [b for b in range(p["batch"]) if b not in upload]
    rest = [b for b in range(p["batch"]) if b not in sweep]
    for key, a32, b32 in (("r_x", x32, y32), ("r_u", u32, v32)):
        assert same(buf[key][upload], widened(b32)[upload]) and same(buf[key][kept], widened(a32)[kept]), key
    for key in OUT:                                             # nobody who is not swept is written
        assert same(got["resident"][key][rest], snap[True][key][rest]), key
    assert same(got["listed"]["status"], got["resident"]["status"][sweep]) and same(got["listed"]["delta_J"], got["resident"]["delta_J"][sweep])
    assert all(s.endswith(":subset") for s in got["listed"]["launch"]), got["listed"]["launch"]
    assert not same(got["resident"]["K"][upload], snap[True]["K"][upload])


# ---- 6. everything at once -------------------------------------------------------------------------------------------------------------
def test_every_option_in_one_call():
    """kp_columns32 + K32 + gain_traj + upload_traj + sweep_traj + r_x32 + r_u32 on panda3 fused, behind a whole call that brought FP32
    columns and FP32 Jacobians; the twin passes the same options and the widened Jacobians as FP64."""
    name, fused = "panda3", True
    p = problem(name)
    x32, u32 = floats(name)
    y32, v32 = floats(name, 11)
    dofs = synth.kp_entry_dofs(p)
    cols = synth.kp_columns(p)
    scaled = cols.copy()
    unit = synth._kp_unit_rows(dofs, p["dof"])
    scaled[unit] -= 1.0
    scaled *= 0.75
    scaled[unit] += 1.0
    c32 = [synth.encode_kp_columns_f32(c, dofs, p["dof"]) for c in (cols, scaled)]
    sweep, upload, gain = [1, 2], [2], [0, 2]
    listed = c32[1][ss.entry_index(p, upload)]
    assert 0 < len(listed) < len(c32[0])

    def scenario(e, new):
        res = {}
        out = call(e, p, new, 3, x32, u32, kp_cols32=pin(e, c32[0]))
        e.sync()
        res["whole"] = grab(e, out)
        out = call(e, p, new, 3, y32, v32, upload=upload, sweep=sweep, gain=gain, K32=True, kp_cols32=pin(e, listed),
                   lam=float(p["lam"]) * np.array([2.0, 0.5]))
        e.sync()
        res["listed"] = grab(e, out, sweep=sweep, gain=gain, K32=True)
        res["resident"] = resident(e)
        return res

    want, got, buf = both(p, fused, scenario)
    assert same(got["listed"]["K"], cast_gains(got["resident"]["K"][gain]))
    assert np.all(want["whole"]["status"] == 0) and np.all(want["listed"]["status"] == 0)
    assert not same(got["resident"]["K"][2], want["whole"]["K"][2]) and same(got["resident"]["K"][0], want["whole"]["K"][0])
    assert same(buf["r_x"][2], widened(y32)[2]) and same(buf["r_x"][:2], widened(x32)[:2])
    assert same(buf["r_u"][2], widened(v32)[2]) and same(buf["r_u"][:2], widened(u32)[:2])


# ---- 7. special values -----------------------------------------------------------------------------------------------------------------
SUB_MIN = np.float32(2.0 ** -149)
SUB_MAX = np.float32(2.0 ** -126 - 2.0 ** -149)
BIG = np.finfo(np.float32).max
SPECIALS = [np.float32(-0.0), SUB_MIN, SUB_MAX, np.finfo(np.float32).tiny, BIG, -BIG]


@functools.lru_cache(maxsize=None)
def special_floats():
    """acrobot5's floats with the special values at the first and the last element of every chunk's slice (three chunks: trajectories
    0 | 1-2 | 3-4) of both arrays, in another order for r_u32"""
    x32, u32 = floats("acrobot5")
    x32, u32 = x32.copy(), u32.copy()
    ends = [(0, 0), (0, -1), (1, 0), (2, -1), (3, 0), (4, -1)]              # (trajectory, element of its rows)
    for a, turn in ((x32, 0), (u32, 3)):
        flat = a.reshape(a.shape[0], -1)
        for i, (b, el) in enumerate(ends):
            flat[b, el] = SPECIALS[(i + turn) % len(SPECIALS)]
    return x32, u32


@pytest.mark.parametrize("pipe_copy", PIPE_COPY, ids=PIPE_IDS)
def test_special_values_widen_exactly_and_sweep_like_the_twin(pipe_copy, monkeypatch):
    """-0.0, 2^-149, the largest FP32 subnormal, FLT_MIN and +-FLT_MAX at the first and the last element of every chunk's slice of both
    arrays.  On the CPU first: the oracle's pipeline on the widened problem ends every trajectory with status 0 and finite gains --
    with +-FLT_MAX itself, so nothing had to be lowered.  (NaN and +-inf pass through the same conversion by contract, but no sweep is
    held to anything on non-finite Jacobians: not fed here.)"""
    set_pipe_copy(monkeypatch, pipe_copy)
    name, fused = "acrobot5", True
    p = problem(name)
    x32, u32 = special_floats()
    assert 0 < SUB_MIN < SUB_MAX < np.finfo(np.float32).tiny and np.float32(SUB_MIN / 2) == 0
    q = dict(p)
    q["r_x"], q["r_u"] = widened(x32), widened(u32)
    for b in range(p["batch"]):
        o = pipeline.run_trajectory(q, b)
        assert o["status"] == 0 and np.all(np.isfinite(o["K"])) and np.all(np.isfinite(o["k"])), b

    def scenario(e, new):
        out = call(e, p, new, 3, x32, u32)
        e.sync()
        return {"specials": grab(e, out)}

    want, got, buf = both(p, fused, scenario)
    for key, a32 in (("r_x", x32), ("r_u", u32)):
        assert same(buf[key], widened(a32)), key               # numpy's widening, bit for bit: -0 keeps its sign, subnormals their value
        flat = buf[key].reshape(p["batch"], -1)
        assert {float(v) for v in (flat[0, 0], flat[0, -1], flat[1, 0], flat[2, -1], flat[3, 0], flat[4, -1])} == {float(np.float64(v)) for v in SPECIALS}
        assert np.count_nonzero(buf[key] == np.float64(SUB_MIN)) >= 1 and np.float64(SUB_MIN) != 0.0
        assert np.any(np.signbit(buf[key]) & (buf[key] == 0.0))


# ---- 8. consecutive calls without a wait -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe_copy", PIPE_COPY, ids=PIPE_IDS)
@pytest.mark.parametrize("name,fused", [("acrobot5", True), ("panda3", False)], ids=["acrobot5-fused", "panda3-records"])
def test_calls_in_flight_with_different_floats_and_lists(name, fused, pipe_copy, monkeypatch):
    """Two calls, different floats, different upload_traj, no sync in between: a chunk's region of the staging buffer is addressed by the
    chunk, so same-stream order protects it.  (The twin waits between its two calls.)"""
    set_pipe_copy(monkeypatch, pipe_copy)
    p = problem(name)
    x32, u32 = floats(name)
    y32, v32 = floats(name, 11)
    z32, w32 = floats(name, 12)
    first, second = UPLOAD_LISTS[name][4], UPLOAD_LISTS[name][2]          # ends of the batch | a pair straddling a chunk boundary

    def scenario(e, new):
        out = call(e, p, new, 3, x32, u32)
        e.sync()
        res = {"whole": grab(e, out)}
        a = call(e, p, new, 3, y32, v32, upload=first)
        if not new:
            e.sync()
        b = call(e, p, new, 3, z32, w32, upload=second)
        e.sync()
        res["first"], res["second"] = grab(e, a), grab(e, b)
        res["second"]["launch"] = res["first"]["launch"] = launches(e)
        return res

    want, got, buf = both(p, fused, scenario)
    want_x, want_u = widened(x32), widened(u32)
    want_x[first], want_u[first] = widened(y32)[first], widened(v32)[first]
    want_x[second], want_u[second] = widened(z32)[second], widened(w32)[second]
    assert same(buf["r_x"], want_x) and same(buf["r_u"], want_u)
    assert not same(want["first"]["K"], want["second"]["K"]) and np.all(want["second"]["status"] == 0)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_staging_buffer_grows_and_is_shared_with_the_explicit_calls(fused):
    """The explicit partial FP32 upload reserves the staging buffer for one trajectory; the streamed call behind it has to grow it to
    the whole batch, and another explicit upload follows the chunks, with no kpilqr_sync in between.  The twin makes the FP64 calls."""
    name = "panda3"
    p, other = problem(name), problem(name, 11)
    x32, u32 = floats(name)
    y32, v32 = floats(name, 11)
    z32, w32 = floats(name, 12)

    def scenario(e, new):
        e.upload_residuals(None, other["r_x"], other["r_u"])
        if new:
            e.upload_residual_jacobians_f32(z32[[1]], w32[[1]], traj=[1])
        else:
            e.upload_residuals_partial([1], None, widened(z32)[[1]], widened(w32)[[1]])
        out = call(e, p, new, 3, x32, u32)
        if new:
            e.upload_residual_jacobians_f32(y32[[0, 2]], v32[[0, 2]], traj=[0, 2])
        else:
            e.upload_residuals_partial([0, 2], None, widened(y32)[[0, 2]], widened(v32)[[0, 2]])
        behind = call(e, p, new, 3)
        e.sync()
        res = {"streamed": grab(e, out), "behind the explicit upload": grab(e, behind)}
        res["streamed"]["launch"] = res["behind the explicit upload"]["launch"]
        return res

    want, got, buf = both(p, fused, scenario)
    want_x, want_u = widened(x32), widened(u32)
    want_x[[0, 2]], want_u[[0, 2]] = widened(y32)[[0, 2]], widened(v32)[[0, 2]]
    assert same(buf["r_x"], want_x) and same(buf["r_u"], want_u)
    assert not same(want["streamed"]["K"], want["behind the explicit upload"]["K"])
    assert same(want["streamed"]["K"][1], want["behind the explicit upload"]["K"][1])


# ---- 9. state --------------------------------------------------------------------------------------------------------------------------
def base_const(name):
    def prepare(e, p):
        base(e, p)
        e.upload_residual_jacobians_const(problem(name, dense=False)["rx_const"], None)
    return prepare


@pytest.mark.parametrize("name,fused", [("acrobot5", True), ("panda3", False)], ids=["acrobot5-fused", "panda3-records"])
def test_whole_r_x32_ends_the_constant_mode_as_the_fp64_call_does(name, fused):
    p = problem(name)
    assert problem(name, dense=False)["rx_const"] is not None
    x32, _ = floats(name)

    def scenario(e, new):
        res = {}
        out = call(e, p, new, 3)                                 # (the mode has run before it ends)
        e.sync()
        res["constant"] = grab(e, out)
        out = call(e, p, new, 3, x32, None)
        e.sync()
        res["per step"] = grab(e, out)
        out = call(e, p, False, 3, p["r_x"], p["r_u"])           # a later whole FP64 call, kpilqr_iterate_streamed5 on both contexts
        e.sync()
        res["fp64 after"] = grab(e, out)
        return res

    want, got, buf = both(p, fused, scenario, prepare=base_const(name))
    if fused:
        for r in (want, got):
            assert all(":rxc" in s for s in r["constant"]["launch"][:2]), r["constant"]["launch"]
            assert not any(":rxc" in s for s in r["per step"]["launch"][:2]), r["per step"]["launch"]
    assert not same(want["constant"]["K"], want["per step"]["K"])
    # ... and the FP64 call gives a fresh context's bits
    with engine(p, fused) as e:
        base(e, p)
        out = Outputs(e)
        v = out.view
        kw = dict((key, pin(e, np.asarray(p[key], np.float64))) for key in ("r_x", "r_u"))
        e.iterate_streamed(K=v["K"], k=v["k"], cost_pred=v["cost_pred"], delta_J=v["delta_J"], status=v["status"], nchunks=3, eps=p["eps"],
                           lam=pin(e, np.full(p["batch"], float(p["lam"]))), **kw)
        e.sync()
        fresh = grab(e, out)
    equal(got["fp64 after"], fresh, "FP64 after FP32")


# ---- 10. refusals leave the context alone ------------------------------------------------------------------------------------------------
def raw_io6(e, p, out, **fields):
    """kpilqr_stream_io6 with the standard outputs and lambda; fields: r_x / r_u / r_x32 / r_u32 (arrays, or addresses), upload / sweep
    (int32 arrays).  -> (io6, what has to stay alive)"""
    io6 = _lib.StreamIO6()
    io6.struct_size = C.sizeof(_lib.StreamIO6)
    io6.io5.struct_size = C.sizeof(_lib.StreamIO5)
    io6.io5.io4.struct_size = C.sizeof(_lib.StreamIO4)
    io6.io5.io4.io3.struct_size = C.sizeof(_lib.StreamIO3)
    io6.io5.io4.io3.io2.struct_size = C.sizeof(_lib.StreamIO2)
    io = io6.io5.io4.io3.io2.io
    io.eps = float(p["eps"])
    sweep = fields.get("sweep")
    lam = pin(e, np.full(p["batch"] if sweep is None else len(sweep), float(p["lam"])))
    io.lam = lam.ctypes.data
    for key in OUT:
        setattr(io, key, out.view[key].ctypes.data)
    address = lambda a: a if isinstance(a, int) else a.ctypes.data
    for key in ("r_x", "r_u"):
        if fields.get(key) is not None:
            setattr(io, key, address(fields[key]))
        if fields.get(key + "32") is not None:
            setattr(io6, key + "32", address(fields[key + "32"]))
    if fields.get("upload") is not None:
        io6.io5.io4.upload_count, io6.io5.io4.upload_traj = len(fields["upload"]), fields["upload"].ctypes.data
    if sweep is not None:
        io6.io5.sweep_count, io6.io5.sweep_traj = len(sweep), sweep.ctypes.data
    return io6, (lam, fields)


def again(e, p):
    """the iteration on what is resident, through the new call"""
    out = call(e, p, True, 3)
    e.sync()
    return grab(e, out)


def refused(e, p, what, code, word=None, spoil=None, **fields):
    out = Outputs(e)
    io6, keep = raw_io6(e, p, out, **fields)
    if spoil:
        spoil(io6)
    rc = e._L.kpilqr_iterate_streamed6(e._h, C.byref(io6), 100, 3)
    assert rc == code, (what, rc)
    if word:
        assert word in e._L.kpilqr_strerror(e._h).decode(), (what, e._L.kpilqr_strerror(e._h).decode())
    e.sync()
    out.untouched()
    del keep


def test_refused_calls_leave_a_context_without_control_residuals_alone():
    name, fused = "acrobot5", True
    p = problem(name)
    x32, u32 = floats(name)
    B = p["batch"]
    one, two = np.array([1], np.int32), np.array([1, 3], np.int32)
    with engine(p, fused) as e:
        base(e, p)
        out = call(e, p, True, 3, x32, None)                     # a whole r_x; r_u was never given: :ru0
        e.sync()
        before = again(e, p)
        assert ":ru0" in before["launch"][0] and np.all(before["status"] == 0)
        px, pu = pin(e, x32), pin(e, u32)
        dx, du = pin(e, widened(x32)), pin(e, widened(u32))
        shifted = e.pinned(u32.size + 1, np.float32)
        shifted[1:] = u32.reshape(-1)
        assert shifted[1:].ctypes.data == shifted.ctypes.data + 4 and px.ctypes.data % 8 == 0 and pu.ctypes.data % 8 == 0
        pageable = np.array(x32.reshape(-1))
        cases = (
            ("outer struct_size + 8", _lib.ERR_ARG, "struct_size", lambda io6: setattr(io6, "struct_size", C.sizeof(_lib.StreamIO6) + 8), dict(r_x32=px, r_u32=pu)),
            ("outer struct_size - 8", _lib.ERR_ARG, "struct_size", lambda io6: setattr(io6, "struct_size", C.sizeof(_lib.StreamIO6) - 8), dict(r_x32=px, r_u32=pu)),
            ("inner struct_size", _lib.ERR_ARG, "struct_size", lambda io6: setattr(io6.io5, "struct_size", C.sizeof(_lib.StreamIO5) + 8), dict(r_x32=px, r_u32=pu)),
            ("r_x with r_x32", _lib.ERR_ARG, "exclusive", None, dict(r_x=dx, r_x32=px)),
            ("r_u with r_u32", _lib.ERR_ARG, "exclusive", None, dict(r_u=du, r_u32=pu)),
            ("a pageable r_x32", _lib.ERR_ARG, "pinned", None, dict(r_x32=pageable, r_u32=pu)),
            ("r_u32 at a pinned address + 4", _lib.ERR_ARG, "8-byte aligned", None, dict(r_x32=px, r_u32=shifted[1:])),
            ("listed r_u32 on a :ru0 context", _lib.ERR_STATE, "without control residuals", None, dict(r_u32=pu, upload=two)),
            ("r_x32 with sweep_traj but no upload_traj", _lib.ERR_ARG, "come with an upload_traj", None, dict(r_x32=px, sweep=two)),
            ("r_u32 with sweep_traj but no upload_traj", _lib.ERR_ARG, "come with an upload_traj", None, dict(r_u32=pu, sweep=one)),
        )
        for what, code, word, spoil, fields in cases:
            refused(e, p, what, code, word, spoil, **fields)
            equal(again(e, p), before, what)                    # the same bits, the same launch strings (:ru0 among them)
        assert e._L.kpilqr_iterate_streamed6(e._h, None, 100, 3) == _lib.ERR_ARG
        assert np.array_equal(pageable, x32.reshape(-1)) and B == 5
        buf = buffers(e, p)
    assert same(buf["r_x"], widened(x32)) and not np.any(buf["r_u"])


def test_listed_r_x32_is_refused_in_constant_mode_and_the_mode_stays():
    name, fused = "acrobot5", True
    p = problem(name)
    x32, _ = floats(name)
    with engine(p, fused) as e:
        base_const(name)(e, p)
        before = again(e, p)
        assert all(":rxc" in s for s in before["launch"][:2]), before["launch"]
        refused(e, p, "listed r_x32 in constant mode", _lib.ERR_STATE, "constant residual Jacobians", None,
                r_x32=pin(e, x32[[0, 2]]), upload=np.array([0, 2], np.int32))
        equal(again(e, p), before, "after the refused call")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_listed_r_x32_is_refused_before_a_whole_r_x(fused):
    name = "panda3"
    p = problem(name)
    x32, u32 = floats(name)
    res = []
    for refuse in (False, True):
        with engine(p, fused) as e:
            base(e, p)
            if refuse:
                refused(e, p, "listed r_x32 before a whole r_x", _lib.ERR_STATE, "before a whole r_x", None,
                        r_x32=pin(e, x32[[0, 2]]), upload=np.array([0, 2], np.int32))
            out = call(e, p, True, 3, x32, u32)
            e.sync()
            res.append((grab(e, out), buffers(e, p)))
    equal(res[1][0], res[0][0], "behind the refused call")
    assert same(res[1][1]["r_x"], res[0][1]["r_x"]) and same(res[1][1]["r_u"], res[0][1]["r_u"])


def test_refused_on_an_embedded_context(monkeypatch):
    import test_gpu_embed as ge
    ge._set_env(monkeypatch, {})
    p = ge._problem(3, 2, 5, 23, "ragged", False)
    with Engine(3, 2, 23, 5, batch=ge.B, fused=True, embed=True) as e:
        ge._upload(e, p, "cols", False)

        def once():
            e.iterate(p["lam"], 5, orc.alphas(6))
            K, k = e.gains()
            return dict(e.results(), K=K, k=k, launch=[e.last_launch("backward"), e.last_launch("forward")])
        before = once()
        x32 = e.pinned((ge.B, 24, 5, 6), np.float32); x32[...] = 0.5
        with pytest.raises(KpilqrError) as err:
            e.iterate_streamed6(r_x32=x32)
        assert err.value.code == _lib.ERR_STATE and "kpilqr_iterate_streamed6" in str(err.value) and "not on an embedded context" in str(err.value)
        equal(once(), before, "embedded")
