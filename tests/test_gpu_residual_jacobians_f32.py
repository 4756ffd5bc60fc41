"""GPU tests of the FP32 residual-Jacobian upload, kpilqr_upload_residual_jacobians_f32 / kpilqr_upload_residual_jacobians_f32_partial
(residuals_f32.hip).

The yardstick of every case is the FP64 call fed the numpy-WIDENED doubles (astype(float64) of the floats) on a second context of the
same flags: the library's widening must leave the bits that call leaves -- the r_x / r_u device buffers, and K, k, delta_J, status,
cost_pred and U_alpha behind kpilqr_iterate, array_equal -- and the launch strings it leaves.  (What the rounding itself costs is the
CPU side: tests/test_residual_jacobians_f32_abi.py.)"""
import functools

import numpy as np
import pytest

import _residual_jacobians_f32 as rj
from oracle import oracle as orc
from trajoptkp_amd import Engine, _lib, host, synth
from trajoptkp_amd.engine import KpilqrError

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -5
ALPHAS = orc.alphas(6)


# ---- problems -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(name, config_id=None, dense=True):
    if name == "acrobot":            # n = 4, m = 1, nr = 5: r_u has 37 * 5 * 1 = 185 elements per trajectory, odd -- the element path, odd bases
        kw = dict(task="acrobot", T=36, batch=5, min_N=5, config_id=1)
    elif name == "panda":            # r_x has 38 * 14 * 14 = 7448 elements per trajectory: several slices of pairs
        kw = dict(task="panda_reaching", T=37, batch=3, min_N=5, config_id=2)
    elif name == "m_gt_dof":         # (dof, m, nr) = (3, 5, 3)
        kw = dict(task=synth.shape_task(3, 5, 3), T=33, batch=2, min_N=4, config_id=4)
    else:
        raise KeyError(name)
    if config_id is not None:
        kw["config_id"] = config_id
    return synth.make_problem(dense_residuals=dense, **kw)


def _payload(p):
    """(r_x32, r_u32, their exact widenings): what crosses the link, and what the FP64 twin is fed"""
    x32, u32 = synth.residual_jacobians_f32(p)
    q = rj.decoded_twin(p)
    assert np.array_equal(rj.decode(x32), q["r_x"]) and np.array_equal(rj.decode(u32), q["r_u"])
    assert np.count_nonzero(q["r_x"] != p["r_x"]) > p["r_x"].size // 4          # the transport rounds: this is not the FP64 payload again
    return x32, u32, q["r_x"], q["r_u"]


# ---- contexts -----------------------------------------------------------------------------------------------------------------
def _engine(p, fused):
    e = Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=fused)
    if fused:
        assert "fused" in e.backward_variant
    return e


def _base(e, p):
    """Everything but the residual Jacobians: key-points, the FD payload, r and the weights, the nominal controls"""
    e.set_keypoints_rows(p["kp_rows"])
    e.upload_fd(p["job_b"], p["job_t"], p["job_col"], p["job_mode"], p["xplus"], p["xminus"], job_nom=p["job_nom"], xnom=p["xnom"], eps=p["eps"])
    e.upload_residuals(p["r"], None, None, p["w_run"], p["w_term"])
    e.upload_nominal(p["u_nom"], p["ctrl_lim"])


def _buffers(e, p, which=("r_x", "r_u")):
    """The r_x / r_u device buffers.  (kpilqr_device_ptr hands out a writable pointer: reading r_u ends :ru0 on this context, so the
    tests that look at :ru0 read r_x alone.)"""
    import torch
    e.sync()
    out = {}
    for key in which:
        buf = _lib.BUF_R_X if key == "r_x" else _lib.BUF_R_U
        out[key] = torch.as_tensor(e.device_array(buf, p[key].shape), device=f"cuda:{e.device}").cpu().numpy().copy()
    return out


def _iterate(e, p):
    """K, k, delta_J, status, cost_pred, U_alpha behind kpilqr_iterate, and what the two sweeps ran as"""
    e.iterate(p["lam"], 100, ALPHAS)
    res = e.results()
    K, k = e.gains()
    _, U = e.forward_linear(None, want_U=True)             # (the resident alphas: the controls of the iteration's forward sweep)
    return dict(K=K, k=k, delta_J=res["delta_J"], status=res["status"], cost_pred=res["cost_pred"], U_alpha=U,
                launches=np.array([e.last_launch("backward"), e.last_launch("forward")]))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, what):
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), (what, key, got[key] if key == "launches" else None, want[key] if key == "launches" else None)


def _same_buffers(got, want, what):
    for key in want:
        assert np.array_equal(_bits(got[key]), _bits(want[key])), (what, key)


def _raises(code, f, *a, **kw):
    with pytest.raises(KpilqrError) as err:
        f(*a, **kw)
    assert err.value.code == code, err.value


# ---- 1. the whole upload leaves the bits of the FP64 call on the widened doubles ------------------------------------------------------
CASES = [("acrobot", True), ("acrobot", False), ("panda", True), ("panda", False), ("m_gt_dof", False)]      # (m > dof has no fused form)


@pytest.mark.parametrize("name,fused", CASES, ids=[f"{n}-{'fused' if f else 'records'}" for n, f in CASES])
def test_whole_upload_equals_its_fp64_twin(name, fused):
    p = _problem(name)
    x32, u32, dx, du = _payload(p)
    out = []
    for upload in (lambda e: e.upload_residuals(None, dx, du), lambda e: e.upload_residual_jacobians_f32(x32, u32)):
        with _engine(p, fused) as e:
            _base(e, p)
            upload(e)
            out.append((_buffers(e, p), _iterate(e, p)))
    (want_buf, want), (got_buf, got) = out
    assert np.array_equal(_bits(want_buf["r_x"]), _bits(dx)) and np.array_equal(_bits(want_buf["r_u"]), _bits(du))
    _same_buffers(got_buf, want_buf, name)
    assert np.all(want["status"] == 0) and np.any(want["K"] != 0)
    _same(got, want, name)
    for s in got["launches"]:
        assert s and ":rxc" not in s and ":ru0" not in s, s


def test_r_x_alone_keeps_the_context_without_control_residuals():
    """r_u32 = NULL: r_u stays exactly zero and the fused sweeps stay in their :ru0 instantiations, as behind the FP64 call"""
    p = _problem("acrobot")
    x32, _, dx, _ = _payload(p)
    out = []
    for upload in (lambda e: e.upload_residuals(None, dx, None), lambda e: e.upload_residual_jacobians_f32(x32, None)):
        with _engine(p, True) as e:
            _base(e, p)
            upload(e)
            out.append((_buffers(e, p, ("r_x",)), _iterate(e, p)))
    (want_buf, want), (got_buf, got) = out
    _same_buffers(got_buf, want_buf, "r_x alone")
    _same(got, want, "r_x alone")
    assert ":ru0" in got["launches"][0] and ":rxc" not in got["launches"][0], got["launches"]


# ---- 2. the partial upload equals its FP64 twin ------------------------------------------------------------------------------------
PARTIAL = [("acrobot", (1, 3, 4), True), ("acrobot", (1, 3, 4), False), ("acrobot", (0,), True), ("panda", (0, 2), True), ("panda", (0, 2), False)]


@pytest.mark.parametrize("name,traj,fused", PARTIAL, ids=[f"{n}-{'_'.join(map(str, t))}-{'fused' if f else 'records'}" for n, t, f in PARTIAL])
def test_partial_upload_equals_its_fp64_twin(name, traj, fused):
    p0, p1 = _problem(name), _problem(name, config_id=11)           # new Jacobians for the listed trajectories, from another draw
    traj = list(traj)
    kept = [b for b in range(p0["batch"]) if b not in traj]
    x32_0, u32_0, dx0, du0 = _payload(p0)
    x32_1, u32_1, dx1, du1 = _payload(p1)
    assert not np.array_equal(x32_0[traj], x32_1[traj]) and not np.array_equal(u32_0[traj], u32_1[traj])

    def sequence(e, whole, partial):
        _base(e, p0)
        whole(e)
        partial(e)
        return _buffers(e, p0), _iterate(e, p0)

    with _engine(p0, fused) as e:
        want_buf, want = sequence(e, lambda e: e.upload_residuals(None, dx0, du0),
                                  lambda e: e.upload_residuals_partial(traj, None, dx1[traj], du1[traj]))
    with _engine(p0, fused) as e:
        got_buf, got = sequence(e, lambda e: e.upload_residual_jacobians_f32(x32_0, u32_0),
                                lambda e: e.upload_residual_jacobians_f32(x32_1[traj], u32_1[traj], traj=traj))
    for key, new, old in (("r_x", dx1, dx0), ("r_u", du1, du0)):
        assert np.array_equal(_bits(got_buf[key][traj]), _bits(new[traj])), key          # the listed rows arrived ...
        assert np.array_equal(_bits(got_buf[key][kept]), _bits(old[kept])), key          # ... and nobody else's rows were touched
    _same_buffers(got_buf, want_buf, name)
    assert np.all(want["status"] == 0)
    _same(got, want, name)


# ---- 3. special values -----------------------------------------------------------------------------------------------------------------
def test_special_values_widen_exactly():
    """NaN, +-inf, -0, the smallest FP32 subnormal and FP32's largest value at the first and the last element of a trajectory's rows
    and at odd offsets, through the whole and the partial call; the buffers are read back, no sweep runs on them."""
    p = _problem("acrobot")
    B = p["batch"]
    x32, u32, _, _ = _payload(p)
    x32, u32 = x32.copy(), u32.copy()
    sub = np.float32(2.0 ** -149)
    assert 0 < sub < np.finfo(np.float32).tiny and np.float32(sub / 2) == 0
    specials = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0), sub, -sub, np.finfo(np.float32).max]
    for a in (x32, u32):
        flat = a.reshape(B, -1)
        per = flat.shape[1]
        for i, v in enumerate(specials):
            b = i % B
            flat[b, 0 if i < B else 2 * i + 1] = v                 # the first element of a trajectory's rows | an odd offset
            flat[(b + 1) % B, per - 1 if i < B else per - 2 * i] = v      # the last element | an odd (r_u: even) offset from the end
            flat[(b + 2) % B, 7 + 2 * i] = v                       # an odd offset
    assert (u32.reshape(B, -1).shape[1] % 2, x32.reshape(B, -1).shape[1] % 2) == (1, 0)

    def check(got, want32, what):
        want = want32.astype(np.float64)
        nan = np.isnan(want)
        assert np.count_nonzero(nan) >= 3 and np.array_equal(np.isnan(got), nan), what
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), what
        assert np.count_nonzero(got == np.float64(sub)) >= 1 and np.float64(sub) != 0.0, what       # the subnormal kept its value

    with _engine(p, False) as e:
        e.upload_residual_jacobians_f32(x32, u32)
        buf = _buffers(e, p)
        check(buf["r_x"], x32, "whole r_x"); check(buf["r_u"], u32, "whole r_u")
        # the partial call: the same rows, rolled by one trajectory, onto a scattered list
        traj = [1, 3, 4]
        src = [0, 2, 3]
        e.upload_residual_jacobians_f32(x32[src], u32[src], traj=traj)
        buf = _buffers(e, p)
        want_x, want_u = x32.copy(), u32.copy()
        want_x[traj], want_u[traj] = x32[src], u32[src]
        check(buf["r_x"], want_x, "partial r_x"); check(buf["r_u"], want_u, "partial r_u")


def test_rows_past_2_31_elements_land_where_they_belong():
    """64-bit offsets: a batch whose r_x buffer has more than 2^31 elements (17 GB) and whose r_u buffer more than 2^32 bytes, rows
    uploaded for an ordinary trajectory and for the LAST one through the partial call -- two trajectories' floats cross the link.
    The rows arrive at the last trajectory, and the first ten trajectories -- a byte offset cut to 32 bits would land in trajectory 6
    of either buffer -- still hold the zeros the buffers were created with, the ordinary trajectory's rows apart.  (The
    source side of the same arithmetic, i * per of a whole upload, would need 8.6 GB of floats on the host: not run.)"""
    import torch
    dof, m, T, nr = 2, 1, 36, 5
    n, per_x, per_u = 2 * dof, (T + 1) * nr * 2 * dof, (T + 1) * nr * m
    B = 2 ** 31 // per_x + 8
    last = B - 1
    assert last * per_x > 2 ** 31 and last * per_u * 8 > 2 ** 32 and per_u % 2 == 1
    rng = np.random.default_rng(5)
    x32 = rng.standard_normal((2, T + 1, nr, n)).astype(np.float32)
    u32 = rng.standard_normal((2, T + 1, nr, m)).astype(np.float32)
    near = np.arange(10)
    with Engine(dof, m, T, nr, batch=B, fused=True) as e:
        # (a writable pointer to a buffer counts as a whole upload of it: rows of a subset are accepted behind it)
        rx = torch.as_tensor(e.device_array(_lib.BUF_R_X, (B, T + 1, nr, n)), device=f"cuda:{e.device}")
        ru = torch.as_tensor(e.device_array(_lib.BUF_R_U, (B, T + 1, nr, m)), device=f"cuda:{e.device}")
        e.upload_residual_jacobians_f32(x32, u32, traj=[1, last])
        e.sync()
        for buf, a32 in ((rx, x32), (ru, u32)):
            low, high = buf[:10].cpu().numpy(), buf[B - 3:].cpu().numpy()
            assert np.array_equal(low[1], a32[0].astype(np.float64)) and np.array_equal(high[2], a32[1].astype(np.float64))
            assert not np.any(low[near != 1]) and not np.any(high[:2])
        del rx, ru


# ---- 4. refusals leave the context alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_refused_calls_leave_the_context_alone(fused):
    p = _problem("acrobot")
    B = p["batch"]
    x32, u32, _, _ = _payload(p)
    with _engine(p, fused) as e:                                     # a context that never saw a refused call
        _base(e, p)
        e.upload_residual_jacobians_f32(x32, None)
        want = _iterate(e, p)
    with _engine(p, fused) as e:
        _base(e, p)
        _raises(ERR_STATE, e.upload_residual_jacobians_f32, x32[[1, 3]], None, traj=[1, 3])            # r_x of a subset before a whole r_x
        assert "before a whole r_x" in str(e._L.kpilqr_strerror(e._h).decode())
        e.upload_residual_jacobians_f32(None, None)                                                    # NULL / NULL: nothing happens
        e.upload_residual_jacobians_f32(None, None, traj=[0, 2])
        e.upload_residual_jacobians_f32(x32, None)
        _raises(ERR_STATE, e.upload_residual_jacobians_f32, None, u32[[1, 3]], traj=[1, 3])            # r_u rows on a context without control residuals
        assert "without control residuals" in str(e._L.kpilqr_strerror(e._h).decode())
        for bad in ([3, 1], [1, 1], [-1, 2], [1, B]):                                                  # the `traj` rules of the _partial family
            _raises(ERR_ARG, e.upload_residual_jacobians_f32, x32[:2], None, traj=bad)
        assert e._L.kpilqr_upload_residual_jacobians_f32_partial(e._h, 2, None, x32.ctypes.data, None) == ERR_ARG
        assert e._L.kpilqr_upload_residual_jacobians_f32_partial(e._h, -1, None, None, None) == ERR_ARG
        e.upload_residual_jacobians_f32(x32[:0], None, traj=[])                                        # nobody is listed: nothing to do
        _same(_iterate(e, p), want, "after the refused calls")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_partial_r_x_is_refused_in_constant_jacobian_mode(fused):
    p = _problem("acrobot", dense=False)
    assert p["rx_const"] is not None
    x32, _ = synth.residual_jacobians_f32(_problem("acrobot"))
    with _engine(p, fused) as e:
        _base(e, p)
        e.upload_residual_jacobians_const(p["rx_const"], None)
        want = _iterate(e, p)
    with _engine(p, fused) as e:
        _base(e, p)
        e.upload_residual_jacobians_const(p["rx_const"], None)
        _raises(ERR_STATE, e.upload_residual_jacobians_f32, x32[[0, 2]], None, traj=[0, 2])
        assert "constant residual Jacobians" in str(e._L.kpilqr_strerror(e._h).decode())
        got = _iterate(e, p)
    _same(got, want, "after the refused call")
    if fused:
        assert ":rxc" in got["launches"][0], got["launches"]


# ---- 5. mode changes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_whole_f32_r_x_ends_constant_jacobian_mode_as_the_fp64_call_does(fused):
    pc, p = _problem("acrobot", dense=False), _problem("acrobot")
    x32, _, dx, _ = _payload(p)
    out = []
    for upload in (lambda e: e.upload_residuals(None, dx, None), lambda e: e.upload_residual_jacobians_f32(x32, None)):
        with _engine(p, fused) as e:
            _base(e, p)
            e.upload_residual_jacobians_const(pc["rx_const"], None)
            e.iterate(p["lam"], 100, ALPHAS)                        # (the mode has run before it ends)
            upload(e)
            got = _iterate(e, p)
            out.append((got, _buffers(e, p, ("r_x",))))
    (want, want_buf), (got, got_buf) = out
    _same(got, want, "out of the constant mode")
    _same_buffers(got_buf, want_buf, "out of the constant mode")
    assert np.array_equal(_bits(got_buf["r_x"]), _bits(dx))
    assert ":rxc" not in got["launches"][0], got["launches"]
    # ... and rows of a subset are accepted from here on, as behind a whole FP64 r_x
    with _engine(p, fused) as e:
        _base(e, p)
        e.upload_residual_jacobians_const(pc["rx_const"], None)
        e.upload_residual_jacobians_f32(x32, None)
        e.upload_residual_jacobians_f32(x32[[1]], None, traj=[1])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_fp64_upload_after_an_f32_upload_gives_a_fresh_context_s_bits(fused):
    p = _problem("panda")
    x32, u32, _, _ = _payload(p)
    with _engine(p, fused) as e:
        _base(e, p)
        e.upload_residuals(None, p["r_x"], p["r_u"])
        want = _iterate(e, p)
    with _engine(p, fused) as e:
        _base(e, p)
        e.upload_residual_jacobians_f32(x32, u32)
        rounded = _iterate(e, p)
        e.upload_residuals(None, p["r_x"], p["r_u"])
        got = _iterate(e, p)
    _same(got, want, "FP64 after FP32")
    assert not np.array_equal(rounded["K"], want["K"])              # (and the FP32 payload is another one)


# ---- 6. the host classes -----------------------------------------------------------------------------------------------------------------
HOST_KW = dict(T=100, min_N=5, max_iter=6, min_iter=2, torque_weight=1e-3)
ACRO = dict(n=4, m=1, nr=5)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_host_class_f32_jacobians_equal_the_run_on_the_widened_doubles(fused):
    base = "set_interval+" + ("fused" if fused else "unfused")
    f64 = host.run_acrobot(method=base, **HOST_KW)
    twin = host.run_acrobot(method=base + "+hostf32resjac", **HOST_KW)       # rounded alike, widened on the host, uploaded as FP64
    f32 = host.run_acrobot(method=base + "+f32resjac", **HOST_KW)
    assert f32["iterations"] == twin["iterations"] and f32["iterations"] >= 2
    assert np.array_equal(f32["cost_history"], twin["cost_history"]) and np.array_equal(f32["U"], twin["U"])
    assert np.array_equal(f32["K0"], twin["K0"])
    assert f32["cost_history"][-1] < f32["cost_history"][0]
    assert f32["per_step_jacobian_uploads"] == twin["per_step_jacobian_uploads"] >= 1
    # the Jacobians' bytes are halved, r's are not
    rows = (HOST_KW["T"] + 1) * ACRO["nr"]
    L = twin["per_step_jacobian_uploads"]
    assert twin["residual_bytes_uploaded"] == L * rows * 8 * (1 + ACRO["n"] + ACRO["m"])
    assert f32["residual_bytes_uploaded"] == L * rows * (8 + 4 * (ACRO["n"] + ACRO["m"]))
    assert f64["residual_bytes_uploaded"] == f64["per_step_jacobian_uploads"] * rows * 8 * (1 + ACRO["n"] + ACRO["m"])
    # a task with constant residual Jacobians ignores the option
    const = host.run_acrobot(method=base + "+constjac", **HOST_KW)
    both = host.run_acrobot(method=base + "+constjac+f32resjac", **HOST_KW)
    assert both["per_step_jacobian_uploads"] == 0 and np.array_equal(both["U"], const["U"])
    assert both["residual_bytes_uploaded"] == const["residual_bytes_uploaded"]


SHIM = [("set_interval", np.array([[3.1415, 0.3], [2.6, -0.4], [3.5, 0.1], [1.2, 0.8]]), HOST_KW, True),
        ("set_interval", np.array([[3.1415, 0.3], [2.6, -0.4], [3.5, 0.1], [1.2, 0.8]]), HOST_KW, False),
        # the starts and settings of tests/test_gpu_partial_inputs.py's shim test: steps are rejected, subsets re-linearise
        ("adaptive_accel", np.array([[3.1415, 0.3], [2.6, -0.4], [3.5, 0.1], [1.2, 0.8], [0.4, -1.1], [2.9, 0.9]]),
         dict(T=120, min_N=3, max_iter=9, min_iter=2, torque_weight=1e-3), True)]


@pytest.mark.parametrize("method,q0s,kw,fused", SHIM, ids=["set_interval-fused", "set_interval-records", "adaptive_accel-fused"])
def test_batch_shim_f32_jacobians_equal_the_run_on_the_widened_doubles(method, q0s, kw, fused):
    twin = host.run_acrobot_batch(q0s, method=method + "+hostf32resjac", fused=fused, **kw)
    f32 = host.run_acrobot_batch(q0s, method=method + "+f32resjac", fused=fused, **kw)
    assert np.array_equal(f32["iterations"], twin["iterations"]) and f32["iterations"].max() >= 2
    assert np.array_equal(f32["cost_history_raw"], twin["cost_history_raw"]) and np.array_equal(f32["U"], twin["U"])
    assert np.array_equal(f32["keypoint_entries"], twin["keypoint_entries"]) and np.array_equal(f32["final_lambda"], twin["final_lambda"])
    rows = (kw["T"] + 1) * ACRO["nr"]
    per64, per32 = rows * 8 * (1 + ACRO["n"] + ACRO["m"]), rows * (8 + 4 * (ACRO["n"] + ACRO["m"]))
    L, rest = divmod(twin["residual_bytes_uploaded"], per64)         # trajectory linearisations whose residuals went up
    assert rest == 0 and L >= len(q0s)
    assert f32["residual_bytes_uploaded"] == L * per32
    print(f"{method}: {L} trajectory linearisations of {len(twin['keypoint_entries']) * len(q0s)}, {f32['residual_bytes_uploaded']} against {twin['residual_bytes_uploaded']} bytes")
    if method == "adaptive_accel":
        assert L < len(twin["keypoint_entries"]) * len(q0s)          # subsets re-linearised: the partial call ran
