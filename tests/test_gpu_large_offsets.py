"""Every sweep family held to the oracle where offsets need more than 32 bits (tests/_large_offsets.py; the table is checked on the
CPU by tests/test_large_offset_table.py).

A case is UNIQ distinct trajectories replicated over a batch whose step records (materialising families) or per-step r_x (fused ones)
are past 2^31 ELEMENTS and whose K is past 2^32 bytes.  One context per case; the variant and launch strings are asserted.  Then
  1. status 0 everywhere;
  2. the LAST UNIQ trajectories -- the highest offsets, one per seed -- have K, k, delta_J, cost_pred and U_alpha within the suite's
     1e-9 of oracle.pipeline.run_trajectory (the gains through the partial download);
  3. on the device, every trajectory's K, k, delta_J, cost_pred, U_alpha and step records are bit-identical to the same-seed
     trajectory of that last group: a high store that wrapped into a low trajectory, or a high load that fetched a low one, breaks it.
The listed route (kpilqr_update_keypoints and the _partial calls with the list {1, B - 2, B - 1}) runs behind it on one fused context
and on one context with records.  The last section is the in-trajectory limit of the state / cost wave forward sweep.

Every case prints one line: buffer sizes, wall time, worst error against the oracle (profiles/large_offsets.txt)."""
import time

import numpy as np
import pytest

import _large_offsets as LO
import _shape_run as R
import _shapes as S
from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import Engine, _lib, synth

pytestmark = pytest.mark.gpu

UNIQ = LO.UNIQ
ALPHAS = orc.alphas(LO.N_ALPHA)
CHUNK = 1 << 29                         # bytes of a buffer compared per step on the device


def _dev(e):
    return f"cuda:{e.device}"


def _view(e, which, shape, typestr="<f8"):
    import torch
    return torch.as_tensor(e.device_array(which, shape, typestr), device=_dev(e))


def _tile_on_device(e, which, small, reps):
    """small [UNIQ]... -> the context's buffer [reps * UNIQ]..., replica after replica"""
    import torch
    dst = _view(e, which, (reps * small.shape[0],) + small.shape[1:])
    src = torch.from_numpy(np.ascontiguousarray(small)).to(_dev(e)).reshape(1, -1)
    dst.view(reps, -1).copy_(src.expand(reps, -1))


def _skip_unless_room(c):
    import torch
    need = LO.total_bytes(c) + LO.HEADROOM
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{c['name']}: {free} bytes of device memory are free, the case needs {need} (its table size {LO.total_bytes(c)} + {LO.HEADROOM})")


def _upload(e, c, p):
    """The inputs of the whole batch: lists and payload replicated on the host (they are small), the per-trajectory arrays on the device."""
    reps = c["reps"]
    e.set_keypoints(*LO.tiled_csr(p, reps))
    if c["payload"] == "kp_ordered":
        xp, xm, mode = synth.kp_ordered_payload(p)
        e.upload_fd_kp(e.fd_kp_slab(np.tile(xp, (reps, 1, 1)), np.tile(xm, (reps, 1, 1)), np.tile(mode, reps), pinned=False), eps=p["eps"])
    else:
        j = LO.tiled_jobs(p, reps)
        e.upload_fd(j["job_b"], j["job_t"], j["job_col"], j["job_mode"], j["xplus"], j["xminus"], job_nom=j["job_nom"], xnom=j["xnom"], eps=p["eps"])
    e.upload_residuals(None, None, None, p["w_run"], p["w_term"])
    _tile_on_device(e, _lib.BUF_RESIDUALS, p["r"], reps)
    if c["rx"] == "const":
        e.upload_residual_jacobians_const(p["rx_const"], None)
    else:
        _tile_on_device(e, _lib.BUF_R_X, p["r_x"], reps)
        _tile_on_device(e, _lib.BUF_R_U, p["r_u"], reps)
    e.upload_nominal(None, p["ctrl_lim"])
    _tile_on_device(e, _lib.BUF_U_NOM, p["u_nom"], reps)
    e.sync()


def _stages(e, c):
    """What the family needs in front of its backward sweep (tests/_shape_run.py::_backward)."""
    bv = e.backward_variant
    if not (bv == "mfma_f64_t1_fused" and c["payload"] == "kp_ordered"):
        e.fd_difference()
    if "fused" not in bv:
        e.interpolate()
        if not bv.endswith("_a6"):
            e.cost_derivs()


def _check_launch(e, c, n_simd):
    bv, fv, lb, lf = LO.EXPECT[c["name"]]
    g = R._launched(e)
    assert g["variants"] == (bv, fv), g
    R._check_dispatch(c, g, n_simd)
    assert lb in g["launch"][0] + ":" and lf in g["launch"][1] + ":", g["launch"]
    return g["launch"]


def _replicas_differ(t, reps, skip_rows=(), want=None):
    """t: a device tensor [reps * UNIQ]...  Compares every replica (a row of UNIQ trajectories) with `want` (default: the last one) bit by
    bit, in chunks; returns the number of rows that differ.  skip_rows: replicas left out (the listed route's)."""
    import torch
    v = t.reshape(reps, -1)
    v = v.view(torch.int64) if v.dtype == torch.float64 else v
    want = v[reps - 1] if want is None else (want.reshape(-1).view(torch.int64) if want.dtype == torch.float64 else want.reshape(-1))
    rows = max(1, CHUNK // max(v.shape[1] * v.element_size(), 1))
    keep = torch.ones(reps, dtype=torch.bool, device=v.device)
    for r in skip_rows:
        keep[r] = False
    bad = 0
    for i in range(0, reps, rows):
        diff = (v[i:i + rows] != want).any(dim=1) & keep[i:i + rows]
        bad += int(diff.sum())
    return bad


def _device_buffers(e, c):
    """name -> device view [B]... of the outputs that are held bit by bit (the records: of a context that has them)"""
    B, T, n, m = c["batch"], c["T"], 2 * c["dof"], c["m"]
    out = dict(K=_view(e, _lib.BUF_K, (B, T * n * m)), k=_view(e, _lib.BUF_k, (B, T * m)), delta_J=_view(e, _lib.BUF_DELTA_J, (B, 1)),
               cost_pred=_view(e, _lib.BUF_COST_PRED, (B, c["n_alpha"])), status=_view(e, _lib.BUF_STATUS, (B, 1), "<i4"))
    if not LO.is_fused(c):
        out["records"] = _view(e, _lib.BUF_STEP_RECORDS, (B, T * S.rec_stride(n, m)))
    return out


def _errors(K, k, dJ, cost, U, o):
    return dict(K=R._rel(K, o["K"]), k=R._rel(k, o["k"]), delta_J=abs(dJ - o["delta_J"]) / max(abs(o["delta_J"]), 1e-300),
                cost=R._rel(cost, o["cost_pred"]), U=R._rel(U, o["U_alpha"]))


# ---- the listed route ---------------------------------------------------------------------------------------------------------------
def _listed_route(e, c, p, launch):
    """kpilqr_update_keypoints, the partial payload / residual / nominal uploads, fd_interpolate_partial / cost_derivs_partial,
    backward_partial / forward_linear_partial and download_gains_partial (FP64 and FP32) with the list {1, B - 2, B - 1}: the three get
    fresh seeds and new lists and are held to the oracle; every other trajectory keeps the bits it had (those of its replica in the
    second group of UNIQ, which the list does not touch and whose bits are taken before)."""
    import torch
    B, reps = c["batch"], c["reps"]
    traj = [1, B - 2, B - 1]
    q = LO.problem(c, listed=True)
    refs = [pipeline.run_trajectory(q, i, n_alpha=c["n_alpha"], want_U=True) for i in range(3)]
    assert all(o["status"] == 0 for o in refs)
    bufs = _device_buffers(e, c)
    before = {name: t[UNIQ:2 * UNIQ].clone() for name, t in bufs.items()}           # replica 1: nobody of the list is in it
    offs, times = LO.dof_csr(q)
    e.update_keypoints(traj, offs, times)
    xp, xm, mode = synth.kp_ordered_payload(q)
    e.upload_fd_kp_partial(traj, e.fd_kp_slab(xp, xm, mode), eps=q["eps"])
    e.upload_residuals_partial(traj, q["r"], q["r_x"], q["r_u"])
    e.upload_nominal_partial(traj, q["u_nom"])
    if not LO.is_fused(c):
        e.fd_interpolate_partial(traj)
        e.cost_derivs_partial(traj)
    st, dJ = e.backward_partial(traj, q["lam"], 100)
    cost, U = e.forward_linear_partial(traj, ALPHAS, want_U=True)
    K, k = e.gains(traj=traj)
    K32, _ = e.gains(traj=traj, want_k=False, f32=True)
    assert np.all(st == 0), st
    worst = 0.0
    for i, o in enumerate(refs):
        errs = _errors(K[i], k[i], dJ[i], cost[i], U[i], o)
        worst = max(worst, max(errs.values()))
        assert max(errs.values()) <= R.RTOL, (c["name"], "listed", traj[i], errs)
    assert K32.dtype == np.float32 and np.array_equal(K32.view(np.uint32), K.astype(np.float32).view(np.uint32))
    assert e.last_launch("backward").split(":")[0] == launch[0].split(":")[0]
    # the device holds the listed trajectories' new gains at their places ...
    for i, b in enumerate(traj):
        assert np.array_equal(bufs["K"][b].cpu().numpy().view(np.uint64), K[i].reshape(-1).view(np.uint64)), b
    # ... and everybody else what they had: replica 1 its bits of before, every other replica replica 1's; in the first and the last
    # replica the listed trajectories are left out
    for name, t in bufs.items():
        assert torch.equal(t[UNIQ:2 * UNIQ], before[name]), (c["name"], "listed", name)
        assert _replicas_differ(t, reps, skip_rows=(0, reps - 1), want=before[name]) == 0, (c["name"], "listed", name)
        per = t.shape[1]
        edge = torch.cat([t[:UNIQ], t[B - UNIQ:]]).reshape(2, UNIQ, per)
        for row, listed_here in ((0, (1,)), (1, (UNIQ - 2, UNIQ - 1))):
            for b in range(UNIQ):
                kept = torch.equal(edge[row, b], before[name][b])
                assert kept == (b not in listed_here or name == "status"), (c["name"], "listed", name, row, b)
    return worst


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LO.CASES, ids=LO.case_id)
def test_family_past_32_bit_offsets(c, monkeypatch):
    import torch
    _skip_unless_room(c)
    t0 = time.perf_counter()
    B, reps, T, m = c["batch"], c["reps"], c["T"], c["m"]
    p = LO.problem(c)
    refs = [pipeline.run_trajectory(p, u, n_alpha=c["n_alpha"], want_U=True) for u in range(UNIQ)]
    assert all(o["status"] == 0 for o in refs)
    t_ref = time.perf_counter() - t0
    R._set_env(c, monkeypatch)
    e = Engine(c["dof"], m, T, c["nr"], batch=B, n_alpha=c["n_alpha"], fused=bool(c["flags"] & S.FLAG_FUSED),
               tiled=bool(c["flags"] & S.FLAG_TILED), generic=bool(c["flags"] & S.FLAG_GENERIC))
    try:
        _upload(e, c, p)
        _stages(e, c)
        status, dJ = e.backward(p["lam"], 100)
        cost, U = e.forward_linear(ALPHAS, want_U=True)
        launch = _check_launch(e, c, R._n_simd())
        # 1. status 0 everywhere
        assert not np.any(status), (c["name"], np.nonzero(status)[0][:8])
        # 2. the last UNIQ trajectories against the oracle
        last = list(range(B - UNIQ, B))
        K, k = e.gains(traj=last)
        worst = {}
        for i, b in enumerate(last):
            errs = _errors(K[i], k[i], dJ[b], cost[b], U[b], refs[b % UNIQ])
            worst = {key: max(worst.get(key, 0.0), v) for key, v in errs.items()}
            assert max(errs.values()) <= R.RTOL, (c["name"], b, launch, errs)
        # 3. every trajectory bit-identical to its seed's trajectory of the last group
        bufs = _device_buffers(e, c)
        for name, t in bufs.items():
            assert _replicas_differ(t, reps) == 0, (c["name"], name, launch)
        Ub = U.reshape(reps, -1).view(np.uint64)
        assert np.array_equal(Ub, np.broadcast_to(Ub[-1], Ub.shape)), (c["name"], "U_alpha")
        assert np.array_equal(np.asarray(dJ).reshape(reps, UNIQ).view(np.uint64), np.broadcast_to(np.asarray(dJ)[-UNIQ:].view(np.uint64), (reps, UNIQ)))
        del Ub, U
        listed = _listed_route(e, c, p, launch) if c["listed"] else None
        del bufs
    finally:
        e.close()
        torch.cuda.empty_cache()
    sizes = ", ".join(f"{name} {b['bytes'] / 1e9:.2f}" for name, b in LO.buffers(c).items() if b["bytes"] >= 2 ** 31)
    print(f"\nLARGE {c['name']}: B={B} T={T} total {LO.total_bytes(c) / 1e9:.2f} GB ({sizes}); {launch[0]} | {launch[1]}; "
          f"wall {time.perf_counter() - t0:.1f} s (oracle {t_ref:.1f} s); worst error " + ", ".join(f"{k_} {v:.1e}" for k_, v in worst.items())
          + (f"; listed route worst {listed:.1e}" if listed is not None else ""))


# ---- the in-trajectory limit of the state / cost wave forward sweep -------------------------------------------------------------------
def _fsc_problem(T):
    """One trajectory of the widest two-tile shape, (n, m) = (30, 8), key-points every 500 steps, dense residual Jacobians."""
    d = LO.FSC_SHAPE
    return synth.make_problem(task=synth.shape_task(d["dof"], d["m"], d["nr"]), T=T, batch=1, min_N=500, dense_residuals=True, one_sided_frac=0.1,
                              config_id=LO.CONFIG_ID)


def run_fsc_horizon(T, monkeypatch):
    """The forward sweep over the alphas at horizon T with KPILQR_TILED_FSC = 1 -> (forward launch string, errors of cost_pred and
    U_alpha against a float64 rollout of the linearised closed loop, seconds of that rollout).  The reference is the C oracle's
    forward_linear (oracle/kpilqr_oracle.c) fed the A, B, cost derivatives and gains READ BACK from the device, so that the forward
    sweep alone is judged.  Measured on a CPU at T = 125 204 on the oracle's own A, B and gains: 2.4 s, against 12.7 s of the numpy
    rollout of oracle/crosscheck.py (np_forward); the two agree to 3e-16 on cost_pred and 1e-16 on U_alpha, so the faster one is used."""
    p = _fsc_problem(T)
    c = dict(S._case(p["dof"], p["m"], p["nr"], 0, {"KPILQR_TILED_FSC": "1"}, T=T, batch=1), rx_const=False)
    R._set_env(c, monkeypatch)
    with R._engine(c, p) as e:
        st, _ = R._backward(e, c, p)
        assert st[0] == 0
        cost, U = e.forward_linear(orc.alphas(6), want_U=True)
        launch = e.last_launch("forward")
        A, B = e.get_AB()
        l_x, l_xx, l_u, l_uu = e.get_cost_derivs()
        K, k = e.gains()
    t0 = time.perf_counter()
    want_cost, want_U = orc.forward_linear(p["n"], p["m"], T, orc.alphas(6), A[0], B[0], K[0], k[0], l_x[0], l_xx[0], l_u[0], l_uu[0], p["u_nom"][0],
                                           p["ctrl_lim"], want_U=True)
    dt = time.perf_counter() - t0
    errs = dict(cost=R._rel(cost[0], want_cost), U=R._rel(U[0], want_U))
    print(f"\nFSC T={T}: {launch}; cost_pred error {errs['cost']:.2e}, U_alpha error {errs['U']:.2e}; reference rollout {dt:.2f} s")
    return launch, errs


def test_state_cost_waves_at_the_last_horizon_inside_their_limit(monkeypatch):
    launch, errs = run_fsc_horizon(LO.FSC_T_INSIDE, monkeypatch)
    assert launch == "mfma_f64_tiled:state_cost_waves"
    assert max(errs.values()) <= R.RTOL, errs


def test_first_horizon_beyond_the_state_cost_wave_limit_runs_the_general_form(monkeypatch):
    """T = 125 204: 17 152 B of records per step pass the 0x7fffff00 bytes the form's descriptor holds.  MI355X, before
    forward_tiled_sc_selected looked at the horizon: ":state_cost_waves" ran, status 0, cost_pred off by 1.48e-4 (the last step scored
    on zeros), U_alpha 2.1e-16; with it: the general form, 4.5e-15 and 2.1e-16 (profiles/large_offsets.txt)."""
    launch, errs = run_fsc_horizon(LO.FSC_T_BEYOND, monkeypatch)
    assert launch == "mfma_f64_tiled"                                    # forced or not: the general form
    assert max(errs.values()) <= R.RTOL, errs
