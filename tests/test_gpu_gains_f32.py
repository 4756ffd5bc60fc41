"""GPU tests of the FP32 gain download (kpilqr_download_gains_f32 / _partial, csrc/gains.hip): the conversion bit for bit against
the IEEE cast on crafted values, on real gains against the FP64 download and the oracle, the life of the context's float buffer,
the rejections, and the host shims' opt-in (`+f32gains`).

The reference of the conversion is numpy's float64 -> float32 cast (the C cast: round-to-nearest-even, subnormals kept); the test
checks that reference on the values whose rounding it knows before it trusts it."""
import ctypes as C

import numpy as np
import pytest

from trajoptkp_amd import Engine, _lib, host, synth
from trajoptkp_amd.engine import KpilqrError

pytestmark = pytest.mark.gpu

# (dof, m, T, batch): 1666 elements per trajectory (2 mod 4) | 8 and 4 elements per trajectory (see SMALLEST) | 612 | a tiled shape
SHAPES = [(7, 7, 17, 5), (2, 1, 2, 3), (1, 1, 2, 3), (6, 3, 17, 4), (10, 7, 17, 3)]
# The smallest trajectory one could ask for is (dof, m, T) = (2, 1, 1), 4 elements, but a context needs a horizon of at least two steps
# (kpilqr_create: T < 2 is KPILQR_ERR_ARG, pinned by tests/test_abi.py).  Its two neighbours stand in: the same (dof, m) at the
# shortest horizon (8 elements) and the 4-element trajectory (1, 1, 2); test_one_step_horizon_is_still_refused holds the reason.
SMALLEST = (2, 1, 1, 3)
FLT_MAX = float(np.finfo(np.float32).max)
SENTINEL32, SENTINEL64 = np.float32(-7.25), -7.25
PAD = 64


def lists_for(batch):
    """whole batch, first, last, a scattered list with an adjacent run, the empty list.  [0, 1, 3] needs four trajectories; a batch of
    three has no list that is both scattered and holds a run, so it gets one of each."""
    return [None, [0], [batch - 1], []] + ([[0, 1, 3]] if batch > 3 else [[0, 2], [1, 2]])


def specials():
    """Values whose FP32 rounding is known by construction."""
    f32 = np.float32
    v = [0.0, -0.0, np.inf, -np.inf, np.nan,
         FLT_MAX, -FLT_MAX,
         FLT_MAX + 2.0 ** 103, -(FLT_MAX + 2.0 ** 103),                    # the first double that rounds above FLT_MAX (a tie, to even: inf)
         np.nextafter(FLT_MAX + 2.0 ** 103, 0.0), -np.nextafter(FLT_MAX + 2.0 ** 103, 0.0),      # the last one that stays FLT_MAX
         2.0 ** -150, -(2.0 ** -150),                                      # half the smallest subnormal: a tie, to even: zero
         np.nextafter(2.0 ** -150, 1.0), -np.nextafter(2.0 ** -150, 1.0),  # the next double above it: the smallest subnormal
         2.0 ** -149, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, 3.5 * 2.0 ** -149,      # subnormal ties with even and odd neighbours
         3.3e-40, -1.1e-42, 1e-45, 7e-46, 2.0 ** -126, np.nextafter(2.0 ** -126, 0.0), 2.0 ** -126 * (1 - 2.0 ** -25)]
    # exact ties in the normal range: a float plus half an ulp, neighbours with even and odd last bits, and the doubles next to the tie
    rng = np.random.default_rng(11)
    bits = rng.integers(0x00800000, 0x7F000000, 24, dtype=np.uint32)
    bits[::2] &= np.uint32(0xFFFFFFFE); bits[1::2] |= np.uint32(1)
    f = bits.view(f32)
    tie = f.astype(np.float64) + np.spacing(f).astype(np.float64) / 2
    sign = np.where(np.arange(len(f)) % 3 == 0, -1.0, 1.0)
    v += list(sign * tie) + list(sign * np.nextafter(tie, np.inf)) + list(sign * np.nextafter(tie, 0.0))
    return np.array(v)


def cast(K):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(K, np.float64).astype(np.float32)


def test_the_reference_cast_rounds_as_ieee_says():
    """numpy's cast is the reference of every comparison below: check it where the answer is known."""
    u = lambda x: cast(np.array([x])).view(np.uint32)[0]
    assert u(2.0 ** -150) == 0 and u(np.nextafter(2.0 ** -150, 1.0)) == 1 and u(1.5 * 2.0 ** -149) == 2 and u(2.5 * 2.0 ** -149) == 2
    assert u(3.3e-40) != 0 and u(-(2.0 ** -150)) == 0x80000000
    assert u(FLT_MAX + 2.0 ** 103) == 0x7F800000 and u(np.nextafter(FLT_MAX + 2.0 ** 103, 0.0)) == 0x7F7FFFFF
    assert u(1.0 + 2.0 ** -24) == 0x3F800000 and u(1.0 + 3 * 2.0 ** -24) == 0x3F800002       # ties to even, down and up
    assert u(1e300) == 0x7F800000 and np.isnan(cast(np.array([np.nan]))[0])


def crafted(rng, shape):
    """normals times 10^U(-50, 50) -- overflow to inf, underflow into the FP32 subnormals and to zero -- with the special values at
    random places (as many as fit into half the array)."""
    N = int(np.prod(shape))
    K = rng.standard_normal(N) * 10.0 ** rng.uniform(-50, 50, N)
    sp = rng.permutation(specials())
    at = rng.permutation(N)[:min(len(sp), N // 2)]
    K[at] = sp[:len(at)]
    return K.reshape(shape)


def inject(e, which, a):
    import torch
    dev = torch.as_tensor(e.device_array(which, a.shape), device=f"cuda:{e.device}")
    dev.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    torch.cuda.synchronize()


def same_f32(got, want):
    """bit for bit, except that a NaN only has to be a NaN"""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def same_f64(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def download_f32(e, traj, want_K=True, want_k=True):
    """The raw calls on arrays with sentinel padding in front of and behind the outputs; returns (K32, k) and checks the padding."""
    nb = e.batch if traj is None else len(traj)
    nK, nk = nb * e.T * e.n * e.m, nb * e.T * e.m
    bufK = np.full(nK + 2 * PAD, SENTINEL32, np.float32); bufk = np.full(nk + 2 * PAD, SENTINEL64)
    pK = C.c_void_p(bufK.ctypes.data + PAD * 4) if want_K else None
    pk = C.c_void_p(bufk.ctypes.data + PAD * 8) if want_k else None
    if traj is None:
        e._ck(e._L.kpilqr_download_gains_f32(e._h, pK, pk))
    else:
        tr = np.ascontiguousarray(traj, np.int32)
        e._ck(e._L.kpilqr_download_gains_f32_partial(e._h, len(tr), tr.ctypes.data_as(C.c_void_p) if len(tr) else None, pK, pk))
    e.sync()
    for buf, s, wanted in ((bufK, SENTINEL32, want_K), (bufk, SENTINEL64, want_k)):
        assert np.all(buf[:PAD] == s) and np.all(buf[-PAD:] == s), "a sentinel around the output was overwritten"
        assert wanted or np.all(buf == s), "an output that was not asked for was written"
    return bufK[PAD:PAD + nK].reshape(nb, e.T, e.n, e.m), bufk[PAD:PAD + nk].reshape(nb, e.T, e.m)


# ---- 1. the conversion, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dof,m,T,batch", SHAPES)
def test_conversion_is_the_ieee_cast_for_every_list(dof, m, T, batch):
    rng = np.random.default_rng(100 * dof + 10 * m + T)
    K = crafted(rng, (batch, T, 2 * dof, m))
    k = rng.standard_normal((batch, T, m)) * 10.0 ** rng.uniform(-50, 50, (batch, T, m))
    assert dof != 7 or (np.isinf(cast(K)).sum() > 10 and (cast(K) == 0).sum() > 10 and np.isnan(K).sum() >= 1)
    with Engine(dof, m, T, 2, batch=batch) as e:
        inject(e, _lib.BUF_K, K); inject(e, _lib.BUF_k, k)
        K64, k64 = e.gains()
        assert same_f64(K64, K) and same_f64(k64, k)
        for traj in lists_for(batch):
            rows = slice(None) if traj is None else np.array(traj, np.int64)
            K32, kk = download_f32(e, traj)
            assert same_f32(K32, cast(K[rows])), (traj, "K32 is not the cast of K")
            kref = e.gains(traj=traj, want_K=False)[1] if traj else k64[rows]         # k: bit-identical to kpilqr_download_gains[_partial]
            assert same_f64(kk, kref), traj
            K32, kk = download_f32(e, traj, want_K=False)                               # K32 = NULL: k only
            assert same_f64(kk, k64[rows])
            K32, kk = download_f32(e, traj, want_k=False)                               # k = NULL: K only
            assert same_f32(K32, cast(K[rows]))
            K32b, kb = e.gains(traj=traj, f32=True)                                     # ... and through Engine.gains
            assert K32b.dtype == np.float32 and kb.dtype == np.float64 and same_f32(K32b, cast(K[rows])) and same_f64(kb, k64[rows])
        Kd, kd = e.gains()                                                              # the resident FP64 gains were only read
        assert same_f64(Kd, K) and same_f64(kd, k)
        assert Kd.dtype == np.float64


def test_one_step_horizon_is_still_refused():
    """(dof, m, T, batch) = (2, 1, 1, 3) would be the smallest trajectory (4 elements); no context of one step exists."""
    dof, m, T, batch = SMALLEST
    with pytest.raises(KpilqrError) as ei:
        Engine(dof, m, T, 2, batch=batch)
    assert ei.value.code == _lib.ERR_ARG


# ---- 2. on real gains -----------------------------------------------------------------------------------------------------------
def _backward(e, p):
    from oracle import oracle as orc
    synth.upload(e, p)
    e.fd_difference(); e.interpolate(); e.cost_derivs()
    status, _ = e.backward(p["lam"], 100)
    assert np.all(status == 0)
    return orc.alphas(6)


def test_real_gains_against_the_fp64_download_and_the_oracle(golden_dir):
    from oracle.crosscheck import GOLDEN
    gold = np.load(f"{golden_dir}/panda_T64.npz")
    p = synth.make_problem(**GOLDEN["panda_T64"])
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"]) as e:              # a run that never calls the FP32 download
        alphas = _backward(e, p)
        K_ref, k_ref = e.gains()
        cost_ref = e.forward_linear(alphas)
        imp_ref = e.dof_importance(1)
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"]) as e:
        alphas = _backward(e, p)
        K32, k = e.gains(f32=True)
        K32p, kp = e.gains(traj=[1], f32=True)
        K64, k64 = e.gains()
        cost = e.forward_linear(alphas)
        imp = e.dof_importance(1)
        K32b, _ = e.gains(f32=True)
    assert same_f32(K32, cast(K64)) and same_f32(K32b, K32) and same_f32(K32p, cast(K64[1:2])) and same_f64(k, k64) and same_f64(kp, k64[1:2])
    for b in range(p["batch"]):
        oK = gold[f"b{b}_K"]
        err = float(np.max(np.abs(K32[b].astype(np.float64) - oK)) / np.max(np.abs(oK)))          # relerr of tests/test_gpu_parity.py
        print(f"trajectory {b}: K32 against the oracle's K: {err:.3e} relative")
        assert err < 1e-6, (b, err)
    assert same_f64(K64, K_ref) and same_f64(k64, k_ref) and same_f64(cost, cost_ref) and same_f64(imp, imp_ref)


# ---- 3. the life of the float buffer --------------------------------------------------------------------------------------------
def test_float_buffer_regrows_and_survives_a_resize():
    rng = np.random.default_rng(3)
    batch = 5
    with Engine(7, 7, 17, 2, batch=batch) as e:
        for dof, m, T in ((7, 7, 17), (10, 7, 19), (6, 3, 17)):         # the context's shape, a larger one, a smaller one
            if (dof, m, T) != (e.dof, e.m, e.T):
                e.resize(dof, m, T)
            K = crafted(rng, (batch, T, 2 * dof, m))
            inject(e, _lib.BUF_K, K)
            for traj in ([1], None, [0, 3], [2, 3, 4], None, [4]):       # small, whole (the buffer grows), small again ...
                K32, _ = e.gains(traj=traj, want_k=False, f32=True)
                K64, _ = e.gains(traj=traj, want_k=False)
                assert same_f64(K64, K[slice(None) if traj is None else traj]) and same_f32(K32, cast(K64)), ((dof, m, T), traj)


# ---- 4. rejections --------------------------------------------------------------------------------------------------------------
def test_bad_lists_are_refused_and_change_nothing():
    rng = np.random.default_rng(4)
    dof, m, T, batch = 6, 3, 17, 4
    K = crafted(rng, (batch, T, 2 * dof, m))
    with Engine(dof, m, T, 2, batch=batch) as e:
        inject(e, _lib.BUF_K, K)
        for bad in ([2, 1], [1, 1], [0, batch], [-1, 0], [batch]):      # unsorted, repeated, out of range (above, below, alone)
            tr = np.array(bad, np.int32)
            out = np.full(len(bad) * T * 2 * dof * m, SENTINEL32, np.float32); outk = np.full(len(bad) * T * m, SENTINEL64)
            rc = e._L.kpilqr_download_gains_f32_partial(e._h, len(tr), tr.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                                        outk.ctypes.data_as(C.c_void_p))
            assert rc == _lib.ERR_ARG, (bad, rc)
            e.sync()
            assert np.all(out == SENTINEL32) and np.all(outk == SENTINEL64), bad          # nothing was enqueued
            with pytest.raises(KpilqrError) as ei:
                e.gains(traj=bad, f32=True)
            assert ei.value.code == _lib.ERR_ARG
            K32, _ = download_f32(e, [1, 3])                                               # a valid call still works
            assert same_f32(K32, cast(K[[1, 3]]))
        assert e._L.kpilqr_download_gains_f32_partial(e._h, -1, None, None, None) == _lib.ERR_ARG
        assert e._L.kpilqr_download_gains_f32_partial(e._h, 1, None, None, None) == _lib.ERR_ARG
        assert same_f64(e.gains()[0], K)


# ---- 5. the host shims ----------------------------------------------------------------------------------------------------------
# Measured on an MI355X box (recorded in profiles/gains_f32.txt): the largest relative deviation of the first iteration's six rollout
# costs from the FP64-gains run is 9.938e-16 -- the first iteration starts from zero controls, its feedback term K (x - x_old) is
# small beside alpha k, and K's 6e-8 hardly reaches the cost.  The acrobot amplifies control perturbations, and another box may round
# the same run differently: the test holds ten times the measured deviation, 9.938e-15.
F32_ROLLOUT_DEVIATION_MEASURED = 9.938e-16
F32_ROLLOUT_BOUND = 10 * F32_ROLLOUT_DEVIATION_MEASURED


def test_single_trajectory_shim_first_iteration_rollouts():
    ref = host.optimise("acrobot", T=100, max_iter=2, min_iter=0)
    got = host.optimise("acrobot", T=100, max_iter=2, min_iter=0, options="+f32gains")
    a, b = ref["trace"][0]["rollout_costs"], got["trace"][0]["rollout_costs"]
    assert len(a) == len(b) == 6 and np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    dev = float(np.max(np.abs(b - a) / np.abs(a)))
    print(f"first iteration, six rollout costs, +f32gains against FP64 gains: largest relative deviation {dev:.3e}")
    assert same_f64(ref["trace"][0]["predicted"], got["trace"][0]["predicted"])           # the device's own results do not depend on the download
    assert dev <= F32_ROLLOUT_BOUND, (dev, F32_ROLLOUT_BOUND)


def test_batch_shim_counts_the_bytes_it_moves():
    q0s = np.array([[3.1415, 0.3], [2.6, -0.4], [3.5, 0.1], [1.2, 0.8]])
    Th, n, m = 100, 4, 1
    kw = dict(T=Th, min_N=5, max_iter=6, min_iter=2, torque_weight=1e-3, fused=True)
    f32 = host.run_acrobot_batch(q0s, method="set_interval+f32gains", **kw)
    f64 = host.run_acrobot_batch(q0s, method="set_interval", **kw)
    assert f32["gain_trajectories_fetched"] >= len(q0s) and f64["gain_trajectories_fetched"] >= len(q0s)
    assert f32["gain_bytes_downloaded"] == f32["gain_trajectories_fetched"] * (Th * n * m * 4 + Th * m * 8)
    assert f64["gain_bytes_downloaded"] == f64["gain_trajectories_fetched"] * (Th * n * m * 8 + Th * m * 8)
    assert np.all(np.isfinite(f32["U"])) and all(h[-1] < h[0] for h in f32["cost_history"])
    # without the option the runner gives what its predecessor (the entry point existing callers were built against) gives, bit for bit
    H = host.load_host()
    B, cap = len(q0s), kw["max_iter"] + 2
    hist = np.zeros((B, cap)); its = np.zeros(B, np.int32); U = np.zeros((B, Th)); stats = np.zeros(8)
    traffic = np.zeros(3 + kw["max_iter"] + 1); inputs = np.zeros(2)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = H.kpilqr_host_run_acrobot_batch4(B, Th, 5, kw["max_iter"], 2, 1e-3, p(q0s), 1, b"set_interval", p(hist), cap, p(its),
                                          p(U), p(stats), p(traffic), len(traffic), p(inputs))
    assert rc == 0
    assert np.array_equal(its, f64["iterations"]) and same_f64(U, f64["U"]) and same_f64(stats, f64["stats"])
    assert all(same_f64(hist[b][hist[b] >= 0], f64["cost_history"][b]) for b in range(B))
    assert int(traffic[1]) == f64["gain_bytes_downloaded"] and int(traffic[0]) == f64["payload_bytes_uploaded"]
