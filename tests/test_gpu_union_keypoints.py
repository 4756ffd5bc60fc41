"""GPU tests of KPILQR_FLAG_UNION_KEYPOINTS (Engine(..., union_keypoints=True)): per-DoF key-point lists re-sampled onto the union
of their trajectory's key-point times, so that the segment-loop (uniform) forms of the one-tile fused sweeps run on a union column
store.  A column at an inserted time is the interpolant kpilqr_interpolate writes there, bit for bit; the sweeps on the union store
are held to the oracle at the project's 1e-9 relative bar for K, k, delta_J and the predicted costs, like the per-DoF forms."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import Engine, synth
from trajoptkp_amd.engine import KpilqrError, rows_to_dof_csr

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ONE_WAVE = {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def union_rows(seed, dof, T, B, dens_lo, dens_hi, shared=None):
    """Per trajectory and DoF a random sorted subset of the steps plus 0 and T-1.  The densities differ per DoF and are rolled per
    trajectory; one DoF has only {0, T-1}; one pair of adjacent key-points (gap 1) is planted; no DoF has a key-point at every
    step.  shared: a trajectory whose DoFs all share one list.  Returns (rows per trajectory, the numpy union per trajectory)."""
    rng = np.random.default_rng(seed)
    dens = rng.uniform(dens_lo, dens_hi, dof)
    dens[0] = dens_hi                                     # (one list carries the union's lower bound whatever the draw)
    dens[dof - 1] = 0.0                                   # one DoF only at 0 and T-1
    rows, unions = [], []
    for b in range(B):
        db = np.roll(dens, b)
        lists = []
        for d in range(dof):
            pts = {0, T - 1} | set(np.nonzero(rng.uniform(size=T) < db[d])[0].tolist())
            lists.append(pts)
        dense = int(np.argmax(db))
        t0 = int(rng.integers(2, T - 3))
        lists[dense] |= {t0, t0 + 1}                      # gap 1
        if shared == b:
            lists = [set(lists[dense])] * dof
        lists = [sorted(s) for s in lists]
        assert all(len(l) < T for l in lists) and any(np.any(np.diff(l) == 1) for l in lists)
        assert shared == b or any(len(l) == 2 for l in lists)
        u = np.unique(np.concatenate([np.asarray(l) for l in lists]))
        assert 0.2 <= len(u) / T <= 0.98, len(u) / T      # a union on every step would never exercise the expansion
        rows.append(synth.rows_from_dof_lists(dof, T, lists)); unions.append(u.astype(np.int32))
    return rows, unions


@functools.lru_cache(maxsize=None)
def problem(name):
    """The problems of this file, each with its oracle results: built once, shared, never changed."""
    if name == "panda":          # tests 1, 2
        rows, unions = union_rows(31, 7, 280, 5, 0.03, 0.3, shared=3)
        p = synth.make_ragged_problem("panda_reaching", 280, rows, config_id=7, dense_residuals=True, one_sided_frac=0.25)
    elif name == "acrobot37":    # test 1: dof 2, one control, odd residual count; T no multiple of anything
        rows, unions = union_rows(32, 2, 37, 3, 0.3, 0.5, shared=1)
        p = synth.make_ragged_problem("acrobot", 37, rows, config_id=8, dense_residuals=True, one_sided_frac=0.25)
    elif name == "acrobot64":    # test 3
        rows, unions = union_rows(33, 2, 64, 3, 0.3, 0.5)
        p = synth.make_ragged_problem("acrobot", 64, rows, config_id=9, dense_residuals=True, one_sided_frac=0.25)
    elif name == "panda_rxc":    # test 4: the task's constant selector Jacobian, r_u = 0
        rows, unions = union_rows(34, 7, 96, 4, 0.03, 0.3)
        p = synth.make_ragged_problem("panda_reaching", 96, rows, config_id=10, dense_residuals=False, one_sided_frac=0.25)
    elif name == "acrobot48":    # test 5: eight seeds
        rows, unions = union_rows(35, 2, 48, 8, 0.3, 0.5)
        p = synth.make_ragged_problem("acrobot", 48, rows, config_id=11, dense_residuals=True, one_sided_frac=0.25)
    elif name == "panda96":      # tests 7, 9, 10
        rows, unions = union_rows(36, 7, 96, 5, 0.03, 0.3)
        p = synth.make_ragged_problem("panda_reaching", 96, rows, config_id=12, dense_residuals=True, one_sided_frac=0.25)
    elif name == "panda96b":     # test 7: other lists, other payload
        rows, unions = union_rows(37, 7, 96, 5, 0.05, 0.25)
        p = synth.make_ragged_problem("panda_reaching", 96, rows, config_id=13, dense_residuals=True, one_sided_frac=0.25)
    else:
        raise KeyError(name)
    return p, unions, tuple(pipeline.run_trajectory(p, b) for b in range(p["batch"]))


def engine(p, union=True, batch=None):
    return Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"] if batch is None else batch, fused=True, union_keypoints=union)


def upload(e, p, payload="kp_ordered", rx_const=False):
    synth.upload(e, p, kp_ordered=payload != "job_lists", rx_const=rx_const)
    if payload == "columns":
        e.upload_kp_columns(e.kp_columns(*synth.kp_ordered_payload(p), eps=p["eps"]))


def iterate(e, p, lam=None, pd=100):
    e.iterate(p["lam"] if lam is None else lam, pd, orc.alphas(6))
    res = e.results(); K, k = e.gains()
    return dict(K=K, k=k, status=res["status"], delta_J=res["delta_J"], cost=res["cost_pred"],
                lb=e.last_launch("backward"), lf=e.last_launch("forward"), ll=e.last_launch("linearise"))


def run(p, union=True, payload="kp_ordered", rx_const=False, lam=None, pd=100):
    with engine(p, union) as e:
        upload(e, p, payload, rx_const)
        return iterate(e, p, lam, pd)


def assert_oracle(got, ref, which=None, label=""):
    """The 1e-9 bar for K, k, delta_J and the predicted costs, trajectory by trajectory; the figures are printed before they are held."""
    worst = dict(K=0.0, k=0.0, delta_J=0.0, cost=0.0)
    for b in (range(len(ref)) if which is None else which):
        o = ref[b]
        assert o["status"] == 0
        worst["K"] = max(worst["K"], relerr(got["K"][b], o["K"])); worst["k"] = max(worst["k"], relerr(got["k"][b], o["k"]))
        worst["delta_J"] = max(worst["delta_J"], abs(got["delta_J"][b] - o["delta_J"]) / abs(o["delta_J"]))
        worst["cost"] = max(worst["cost"], relerr(got["cost"][b], o["cost_pred"]))
    print(f"{label} worst relative difference to the oracle: " + ", ".join(f"{q} {v:.2e}" for q, v in worst.items()))
    assert all(got["status"][b] == 0 for b in (range(len(ref)) if which is None else which)), got["status"]
    assert all(v < RTOL for v in worst.values()), worst


def same_bits(a, b, keys=("K", "k", "delta_J", "cost", "status")):
    for key in keys:
        assert np.array_equal(a[key], b[key]), key


def set_env(monkeypatch, env):
    for key in ("KPILQR_FUSED_WAVES", "KPILQR_FUSED_FWD_WAVES", "KPILQR_FUSED_UNI"):
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)


# ---- 1. union structure ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shared", [("panda", 3), ("acrobot37", 1)])
def test_union_lists_and_columns(name, shared):
    """kpilqr_get_union_keypoints is the numpy union per trajectory; kpilqr_get_union_columns holds, bit for bit, the columns d and
    d + dof of A and d < m of B that kpilqr_interpolate writes on an unflagged context with the same payload, at every union
    time; for the trajectory whose DoFs share one list it is the plain column store."""
    p, unions, _ = problem(name)
    dof, n, m, B = p["dof"], p["n"], p["m"], p["batch"]
    with engine(p, union=False) as e:
        upload(e, p)
        e.fd_difference(); e.interpolate()
        A, Bm = e.get_AB()
        with pytest.raises(KpilqrError) as ei:
            e.get_union_keypoints()                       # the flag is not active on this context
        assert ei.value.code == -5
    with engine(p) as e:
        with pytest.raises(KpilqrError) as ei:
            e.get_union_keypoints()                       # no key-points yet
        assert ei.value.code == -5
        e.set_keypoints_rows(p["kp_rows"])
        with pytest.raises(KpilqrError) as ei:
            e.get_union_columns()                         # no payload resident
        assert ei.value.code == -5
        upload(e, p)
        offs, times = e.get_union_keypoints()
        cols = e.get_union_columns()
        ko, kt = e.get_keypoints()                        # the caller's lists are what they were
    co, ct = rows_to_dof_csr(p["kp_rows"], dof, p["T"])
    assert np.array_equal(ko, co) and np.array_equal(kt, ct)
    assert offs[0] == 0 and np.array_equal(np.diff(offs), [len(u) for u in unions])
    assert np.array_equal(times, np.concatenate(unions))
    assert cols.shape == (dof * offs[-1], 3, n)
    inserted = 0
    for b in range(B):
        u = unions[b]
        for d in range(dof):
            ent = dof * offs[b] + d * len(u) + np.arange(len(u))
            assert np.array_equal(cols[ent, 0], A[b, u, d]) and np.array_equal(cols[ent, 1], A[b, u, d + dof]), (b, d)
            if d < m:
                assert np.array_equal(cols[ent, 2], Bm[b, u, d]), (b, d)
            inserted += len(u) - (co[b * dof + d + 1] - co[b * dof + d])
    assert inserted > 0                                   # the expansion interpolated something
    xp, xm, mode = synth.kp_ordered_payload(p)
    with engine(p, union=False) as e:
        plain = e.kp_columns(xp, xm, mode, eps=p["eps"], pinned=False)["cols"].reshape(-1, 3, n)
    lo, hi = co[shared * dof], co[(shared + 1) * dof]
    assert hi - lo == dof * len(unions[shared])
    got = cols[dof * offs[shared]:dof * offs[shared + 1]]
    kinds = np.ones((dof, 1, 3, 1), bool); kinds[m:, :, 2] = False      # (kind-2 slots of DoFs >= num_ctrl are nobody's)
    mask = np.broadcast_to(kinds, (dof, len(unions[shared]), 3, n)).reshape(-1, 3, n)
    assert np.array_equal(got[mask], plain[lo:hi][mask])


# ---- 2. sweeps against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dispatch", ["one_wave", "default"])
@pytest.mark.parametrize("payload", ["job_lists", "kp_ordered", "columns"])
def test_union_sweeps_match_the_oracle(payload, dispatch, monkeypatch):
    """Panda, T = 280, B = 5, every payload form; one wave per trajectory forced, and the small-batch dispatch -- whose forward
    state / cost pair per-DoF lists never reach without the flag.  Flagged and unflagged contexts both meet the oracle bar; their
    largest difference per quantity is printed (profiles/union_keypoints.txt keeps the figures)."""
    p, _, ref = problem("panda")
    set_env(monkeypatch, ONE_WAVE if dispatch == "one_wave" else {})
    got = run(p, True, payload)
    plain = run(p, False, payload)
    lb, lf = got["lb"], got["lf"]
    if dispatch == "one_wave":
        assert ":w1:kpc:uni" in lb and lb.endswith(":union") and ":w1:uni" in lf and lf.endswith(":union"), (lb, lf)
    else:
        assert ":pairh:" in lb and lb.endswith(":union") and ":pair:uni" in lf and lf.endswith(":union"), (lb, lf)
    assert ":raw" not in lb and ":slopes" not in lb and ":slopes" not in lf
    assert got["ll"] == "kp_union"
    assert ":ragged" in plain["lb"] and ":ragged" in plain["lf"] and ":union" not in plain["lb"] + plain["lf"], (plain["lb"], plain["lf"])
    assert plain["ll"] == "in_sweep"
    print(f"{payload}/{dispatch} flagged vs unflagged: " + ", ".join(f"{q} {relerr(got[q], plain[q]):.2e}" for q in ("K", "k", "delta_J", "cost")))
    assert_oracle(got, ref, label=f"{payload}/{dispatch} union:")
    assert_oracle(plain, ref, label=f"{payload}/{dispatch} per-DoF:")


# ---- 3. odd residual count, one control ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dispatch", ["one_wave", "default"])
def test_union_sweeps_acrobot(dispatch, monkeypatch):
    p, _, ref = problem("acrobot64")
    set_env(monkeypatch, ONE_WAVE if dispatch == "one_wave" else {})
    got = run(p)
    assert got["lb"].endswith(":union") and got["lf"].endswith(":union") and (":w1:" in got["lb"]) == (dispatch == "one_wave"), (got["lb"], got["lf"])
    assert_oracle(got, ref, label=f"acrobot/{dispatch}:")


# ---- 4. constant residual Jacobian --------------------------------------------------------------------------------------------------
def test_union_sweeps_with_the_constant_residual_jacobian(monkeypatch):
    """The :rxc:union leg against the flagged per-step-Jacobian leg at 1e-12 (the project's bar for the resident l_xx tile's other
    accumulation order), both against the oracle."""
    p, _, ref = problem("panda_rxc")
    assert p["rx_const"] is not None and not np.any(p["r_u"])
    set_env(monkeypatch, ONE_WAVE)
    step = run(p)
    const = run(p, rx_const=True)
    assert ":rxc" not in step["lb"] and step["lb"].endswith(":union"), step["lb"]
    assert const["lb"].endswith(":rxc:union") and const["lf"].endswith(":rxc:union"), (const["lb"], const["lf"])
    for q in ("K", "k", "delta_J", "cost"):
        assert relerr(const[q], step[q]) <= 1e-12, (q, relerr(const[q], step[q]))
    assert_oracle(step, ref, label="per-step r_x:")
    assert_oracle(const, ref, label="constant r_x:")


# ---- 5. above #SIMDs / 2 trajectories -------------------------------------------------------------------------------------------------
def test_union_sweeps_above_half_the_simds():
    """520 trajectories (eight seeds tiled): no environment switches, one wave per trajectory both ways."""
    p0, _, ref = problem("acrobot48")
    p = synth.tile_problem(p0, 65)
    assert p["batch"] == 520
    got = run(p)
    assert ":w1:kpc:uni" in got["lb"] and got["lb"].endswith(":union") and ":w1:uni" in got["lf"] and got["lf"].endswith(":union"), (got["lb"], got["lf"])
    assert_oracle(got, ref, label="B=520:")
    for key in ("K", "k", "delta_J", "cost", "status"):
        a = np.asarray(got[key]).reshape((65, 8) + np.asarray(got[key]).shape[1:])
        assert np.array_equal(a, np.broadcast_to(a[:1], a.shape)), key


# ---- 6. uniform lists with the flag set -------------------------------------------------------------------------------------------------
def test_uniform_lists_stay_off_the_union_route():
    p = synth.make_problem(task="panda_reaching", T=64, batch=3, min_N=5, dense_residuals=True, one_sided_frac=0.25)
    outs = []
    for union in (True, False):
        with engine(p, union) as e:
            upload(e, p)
            outs.append(iterate(e, p))
            if union:
                offs, times = e.get_union_keypoints()             # still answers: the union is the list
    for o in outs:
        assert ":union" not in o["lb"] + o["lf"] and ":raw:uni" in o["lb"] and o["ll"] == "in_sweep", (o["lb"], o["lf"], o["ll"])
    same_bits(outs[0], outs[1])
    assert np.array_equal(np.diff(offs), [len(p["kp_times"])] * 3) and np.array_equal(times, np.tile(p["kp_times"], 3))


# ---- 7. invalidation ----------------------------------------------------------------------------------------------------------------------
def test_union_follows_new_payloads_keypoints_and_sizes():
    """One flagged context through: iterate | a second payload on the same key-points | new per-DoF lists and a payload | resize to
    the acrobot and back, upload -- each result bit-identical with a fresh flagged context given only that step's inputs."""
    pa, _, _ = problem("panda96")
    pb, _, _ = problem("panda96b")
    pa2 = dict(pa)
    for key in ("xplus", "xminus", "xnom"):
        pa2[key] = pa[key] * 1.01                       # the same lists, residuals and controls; other columns
    ac, _, _ = problem("acrobot37")
    fresh = [run(q) for q in (pa, pa2, pb, pa)]
    assert not np.array_equal(fresh[0]["K"], fresh[1]["K"]) and not np.array_equal(fresh[0]["K"], fresh[2]["K"])
    with engine(pa) as e:
        upload(e, pa)
        same_bits(iterate(e, pa), fresh[0])
        e.upload_fd_kp(e.fd_kp_slab(*synth.kp_ordered_payload(pa2)), eps=pa2["eps"])      # no new key-points: the union lists stay
        same_bits(iterate(e, pa2), fresh[1])
        upload(e, pb)
        same_bits(iterate(e, pb), fresh[2])
        e.resize(ac["dof"], ac["m"], ac["T"])
        e.resize(pa["dof"], pa["m"], pa["T"])
        upload(e, pa)
        got = iterate(e, pa)
        same_bits(got, fresh[3])
        assert got["lb"].endswith(":union") and np.all(got["status"] == 0)


# ---- 8. PD failure --------------------------------------------------------------------------------------------------------------------------
def test_union_pd_failure_status():
    """Negative running residual weights (l_uu indefinite), a PD check every 10 steps, lambdas below and above what the check needs:
    some trajectories stop mid-horizon.  status equals the unflagged context's entry by entry; the others meet the oracle bar."""
    rows, _ = union_rows(38, 7, 64, 4, 0.03, 0.3)
    p = synth.make_ragged_problem("panda_reaching", 64, rows, config_id=5, dense_residuals=True, one_sided_frac=0.25)
    p["w_run"] = -np.abs(p["w_run"]) - 1.0
    lam = np.array([0.2, 0.3, 0.2, 1.0])
    ref = [pipeline.run_trajectory(p, b, lam=lam[b], pd_stride=10) for b in range(4)]
    ok = [b for b in range(4) if ref[b]["status"] == 0]
    assert 0 < len(ok) < 4, [o["status"] for o in ref]
    got = run(p, True, lam=lam, pd=10)
    plain = run(p, False, lam=lam, pd=10)
    assert got["lb"].endswith(":union")
    assert list(got["status"]) == list(plain["status"]) == [o["status"] for o in ref]
    assert_oracle(got, ref, which=ok, label="PD failure:")


# ---- 9. the streamed call ignores the flag ---------------------------------------------------------------------------------------------------
def test_streamed_call_on_a_flagged_context():
    p, _, _ = problem("panda96")
    B = p["batch"]
    xp, xm, mode = synth.kp_ordered_payload(p)
    outs = []
    for union in (True, False):
        with engine(p, union) as e:
            e.set_keypoints_rows(p["kp_rows"])
            e.upload_residuals(None, None, None, p["w_run"], p["w_term"]); e.upload_nominal(None, p["ctrl_lim"])
            e.forward_linear(orc.alphas(6), fetch=False)
            s = e.fd_kp_slab(xp, xm, mode)
            pin = {}
            for name in ("r", "r_x", "r_u", "u_nom"):
                pin[name] = e.pinned(p[name].shape); pin[name][...] = p[name]
            lam = e.pinned(B); lam[:] = p["lam"]
            K = e.pinned((B, p["T"], p["n"], p["m"])); k = e.pinned((B, p["T"], p["m"])); cp = e.pinned((B, 6))
            dJ = e.pinned(B); st = e.pinned(B, np.int32)
            e.iterate_streamed(fd_kp=s, eps=p["eps"], lam=lam, K=K, k=k, cost_pred=cp, delta_J=dJ, status=st, nchunks=3, **pin)
            e.sync()
            lb, lf = e.last_launch("backward"), e.last_launch("forward")
            assert ":union" not in lb + lf and ":ragged" in lb, (lb, lf)
            outs.append(dict(K=np.array(K), k=np.array(k), cost=np.array(cp), delta_J=np.array(dJ), status=np.array(st)))
            if union:                                          # and the ordinary call behind it takes the union route
                assert iterate(e, p)["lb"].endswith(":union")
    assert np.all(outs[0]["status"] == 0)
    same_bits(outs[0], outs[1])


# ---- 10. KPILQR_FUSED_UNI=0 ----------------------------------------------------------------------------------------------------------------------
def test_general_forms_forced_with_the_flag(monkeypatch):
    p, _, ref = problem("panda96")
    set_env(monkeypatch, dict(ONE_WAVE, KPILQR_FUSED_UNI="0"))
    got = run(p)
    assert ":union" not in got["lb"] + got["lf"] and ":ragged" in got["lb"] and ":ragged" in got["lf"] and got["ll"] == "in_sweep", (got["lb"], got["lf"])
    assert_oracle(got, ref, label="KPILQR_FUSED_UNI=0:")
