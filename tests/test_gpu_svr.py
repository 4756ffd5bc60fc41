"""GPU tests of iLQR_SVR's singular-vector DoF importance on the device (kpilqr_dof_importance_svd, svr.hip) against the
host's ThinSVD / DofImportance (host/SVR.cpp): bit for bit on the lane-per-step form (n <= 16, n * m' <= 128), to 1e-12 of
the largest sum on the wave-per-step form, and to 1e-10 against numpy's LAPACK SVD (oracle.dof_importance_svd) everywhere.
Gains are written straight into the context's K buffer (KPILQR_BUF_K) or come from real backward passes."""
import numpy as np
import pytest

from oracle import oracle as orc
from trajoptkp_amd import Engine, host, synth
from trajoptkp_amd.engine import KpilqrError

pytestmark = pytest.mark.gpu

# (dof, m): the lane-per-step form (bit-identical) on the first three, the wave-per-step form on the others
SHAPES = [(2, 1), (3, 2), (7, 7), (10, 7), (31, 7), (27, 21)]


def lane_form(dof, m):
    mp = 1 << (m - 1).bit_length()
    return 2 * dof <= 16 and m <= 16 and 2 * dof * mp <= 128


def random_gains(rng, B, T, dof, m):
    """K [B][T][n][m] with very different state-column scales per trajectory (as test_host.py's host check)."""
    return rng.standard_normal((B, T, 2 * dof, m)) * np.exp(rng.uniform(-3, 2, (B, 1, 2 * dof, 1)))


def inject(e, K):
    import torch
    dev = torch.as_tensor(e.device_array(1, K.shape), device="cuda")       # KPILQR_BUF_K
    dev.copy_(torch.from_numpy(np.ascontiguousarray(K)))
    torch.cuda.synchronize()


def device_importance(K, dof, m, samplings, **kind):
    B, T = K.shape[:2]
    with Engine(dof, m, T, 2, batch=B, **kind) as e:
        inject(e, K)
        return [e.dof_importance_svd(s) for s in samplings]


def host_importance(K, dof, s):
    return host.dof_importance(K, dof, s, svd=True)[0]


def check_against_host(got, K, dof, m, s):
    for b in range(K.shape[0]):
        ref = host_importance(K[b], dof, s)
        assert np.all(np.isfinite(got[b]))
        if lane_form(dof, m):
            assert np.array_equal(got[b], ref), (dof, m, s, b, np.max(np.abs(got[b] - ref)))
        else:
            assert np.max(np.abs(got[b] - ref)) <= 1e-12 * max(np.max(ref), 1e-300), (dof, m, s, b)


@pytest.mark.parametrize("dof,m", SHAPES)
def test_random_gains_match_host_and_lapack(dof, m):
    rng = np.random.default_rng(1000 * dof + m)
    B, T = 3, 40
    K = random_gains(rng, B, T, dof, m)
    samplings = (1, 3, T - 1, T + 5)
    for s, got in zip(samplings, device_importance(K, dof, m, samplings)):
        check_against_host(got, K, dof, m, s)
        for b in range(B):
            ref = orc.dof_importance_svd(dof, m, T, s, K[b])
            assert np.max(np.abs(got[b] - ref)) <= 1e-10 * np.max(ref), (dof, m, s, b)


@pytest.mark.parametrize("kind", [dict(fused=True), dict(), dict(tiled=True), dict(generic=True)])
def test_every_context_kind(kind):
    rng = np.random.default_rng(7)
    K = random_gains(rng, 2, 30, 7, 7)
    got, = device_importance(K, 7, 7, (2,), **kind)
    check_against_host(got, K, 7, 7, 2)


def test_wide_context():
    rng = np.random.default_rng(21)
    K = random_gains(rng, 2, 12, 27, 21)
    got, = device_importance(K, 27, 21, (1,))
    check_against_host(got, K, 27, 21, 1)


def run_problem(p, samplings, **kind):
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], **kind) as e:
        synth.upload(e, p)
        e.iterate(p["lam"], 100, orc.alphas(6))
        res = e.results()
        K, _ = e.gains()
        return res["status"], K, [e.dof_importance_svd(s) for s in samplings]


@pytest.mark.parametrize("task,kind", [("panda_reaching", dict(fused=True)), ("panda_pushing", dict(tiled=True))])
def test_gains_of_real_backward_passes(task, kind):
    p = synth.make_problem(task=task, T=200, batch=3 if task == "panda_reaching" else 2, min_N=5)
    samplings = (1, 7)
    status, K, got = run_problem(p, samplings, **kind)
    assert np.all(status == 0)
    for s, g in zip(samplings, got):
        check_against_host(g, K, p["dof"], p["m"], s)


@pytest.mark.parametrize("dof,m", [(7, 7), (31, 7)])
def test_zero_steps_and_zero_trajectory(dof, m):
    rng = np.random.default_rng(3)
    K = random_gains(rng, 3, 20, dof, m)
    K[0, ::3] = 0.0
    K[1] = 0.0
    for s, got in zip((1, 2), device_importance(K, dof, m, (1, 2))):
        assert np.all(np.isfinite(got))
        assert np.array_equal(got[1], np.zeros(dof))
        check_against_host(got, K, dof, m, s)


@pytest.mark.parametrize("dof,m", [(7, 7), (3, 2), (31, 7), (27, 21)])
def test_rank_deficient_gains(dof, m):
    rng = np.random.default_rng(11)
    B, T, n = 2, 15, 2 * dof
    r = max(1, m // 3)
    K = np.einsum("btnr,btrm->btnm", rng.standard_normal((B, T, n, r)), rng.standard_normal((B, T, r, m)))
    K[:, :, :, -1] = 0.0                                                   # and one control with no gain at all
    for s, got in zip((1, 4), device_importance(K, dof, m, (1, 4))):
        check_against_host(got, K, dof, m, s)


@pytest.mark.parametrize("dof,m", [(7, 7), (3, 2), (6, 4), (2, 1)])
def test_equal_singular_values_keep_the_hosts_tie_break(dof, m):
    """K[t] with orthogonal rows of equal norm: every singular value ties; the lane form must order the columns as the host's
    stable sort does.  Exactly tied (scaled unit rows: no rotation at all) and tied to rounding (rows of a random orthogonal
    matrix)."""
    rng = np.random.default_rng(5)
    B, T, n = 2, 12, 2 * dof
    K = np.zeros((B, T, n, m))
    for b in range(B):
        for t in range(T):
            if t % 2 == 0:
                rows = rng.permutation(n)[:m]
                K[b, t, rows, np.arange(m)] = 2.5
            else:
                Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
                K[b, t] = 0.75 * Q[:, :m]
    assert lane_form(dof, m)
    for s, got in zip((1, 2), device_importance(K, dof, m, (1, 2))):
        check_against_host(got, K, dof, m, s)


def test_reproducible_and_independent_of_batch_neighbours():
    rng = np.random.default_rng(9)
    for dof, m in ((7, 7), (10, 7)):
        K1 = random_gains(rng, 1, 50, dof, m)
        K5 = random_gains(rng, 5, 50, dof, m)
        K5[2] = K1[0]
        a, b = device_importance(K1, dof, m, (1, 1))
        assert np.array_equal(a, b)
        c, = device_importance(K5, dof, m, (1,))
        assert np.array_equal(c[2], a[0])
    # real backward passes: one trajectory alone and five copies of it (synth.tile_problem)
    p = synth.make_problem(task="panda_reaching", T=120, batch=1, min_N=5)
    _, K1, (a,) = run_problem(p, (1,), fused=True)
    _, K5, (c,) = run_problem(synth.tile_problem(p, 5), (1,), fused=True)
    for b in range(5):
        assert np.array_equal(c[b], host_importance(K5[b], p["dof"], 1))
        if np.array_equal(K5[b], K1[0]):
            assert np.array_equal(c[b], a[0])


def test_full_batch_over_staging_chunks():
    """Panda at B = 1024, T = 3000: the staging holds fewer sampled steps than the horizon, so the sums are carried across
    chunks; 16 distinct trajectories tiled over the batch, every copy must give the same bits and match the host."""
    rng = np.random.default_rng(2024)
    dof, m, T, B = 7, 7, 3000, 1024
    K16 = random_gains(rng, 16, T, dof, m)
    K = np.tile(K16, (B // 16, 1, 1, 1))
    for s in (1, 10):
        got, = device_importance(K, dof, m, (s,), fused=True)
        check_against_host(got[:16], K16, dof, m, s)
        assert np.array_equal(got, np.tile(got[:16], (B // 16, 1)))


def test_thresholds_and_arguments():
    rng = np.random.default_rng(4)
    dof, m, T, B = 7, 7, 30, 3
    K = random_gains(rng, B, T, dof, m)
    with Engine(dof, m, T, 2, batch=B) as e:
        inject(e, K)
        for svd in (True, False):
            sums = e.dof_importance_svd(2) if svd else e.dof_importance(2)
            for b in range(B):
                thr = float(np.median(sums[b]))
                got = e.least_important_dofs(thr, 2, svd=svd)
                _, rem = host.dof_importance(K[b], dof, 2, svd=svd, threshold=thr)
                assert got[b] == list(rem) and len(rem) > 0
        with pytest.raises(KpilqrError):
            e.dof_importance_svd(0)
        with pytest.raises(KpilqrError):
            e.least_important_dofs(1.0, 0, svd=True)


@pytest.mark.parametrize("svd", [True, False])
def test_optimiser_classes_on_their_own_gains(svd):
    dev, ref = host.acrobot_dof_importance(q0s=[[3.1415, 0.3], [3.0, 0.0], [2.8, -0.2]], T=100, iters=3, sampling_k_interval=2, svd=svd)
    assert np.array_equal(dev, ref) and np.all(dev > 0)
    dev, ref = host.acrobot_dof_importance(None, T=100, iters=3, fused=True, svd=svd)
    assert np.array_equal(dev, ref) and np.all(dev > 0)
