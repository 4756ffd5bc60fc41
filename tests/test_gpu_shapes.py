"""Every compiled kernel instantiation against the CPU oracle, at problems of any shape (synth.shape_task), not only the task
table's: the cases of tests/_shapes.py (the dispatch restated, with the smallest and largest shape of every key), each run
through the C ABI -- FD, interpolation, cost, backward, forward over the alphas -- and compared with
oracle.pipeline.run_trajectory.  Each case also asserts the variant (and, for the fused sweeps, the wave form) the table
predicts, so that a shape that silently falls back does not count as covering a kernel."""
import numpy as np
import pytest

import _shapes as S
from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import Engine, synth
from trajoptkp_amd.engine import KpilqrError

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def _n_simd():
    # as kpilqr_create does (kpilqr_api.cpp): SIMDs = CUs x 4
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 4


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def _case_id(c):
    env = ",".join(f"{k.replace('KPILQR_', '').lower()}={v}" for k, v in sorted(c["env"].items()))
    return (f"{c['why']}-d{c['dof']}m{c['m']}r{c['nr']}-T{c['T']}-b{c['batch']}-a{c['n_alpha']}-f{c['flags']}"
            + ("-rxc" if c["rx_const"] else "") + ("" if c["uniform"] else "-ragged") + (f"-{env}" if env else ""))


def _problem(c, batch=None, config_id=4):
    task = synth.shape_task(c["dof"], c["m"], c["nr"])
    batch = c["batch"] if batch is None else batch
    dense = False if c["rx_const"] else True
    if c["uniform"]:
        return synth.make_problem(task=task, T=c["T"], batch=batch, min_N=4, dense_residuals=dense, one_sided_frac=0.1,
                                  config_id=config_id)
    # per-DoF lists that differ whatever the seed: DoF 0 has key-points at the ends only, the last one splits every interval
    rng = np.random.default_rng(1000 * c["dof"] + c["m"])
    rows = [synth.bisect_keypoints(rng, c["dof"], c["T"], 2, np.linspace(0.0, 1.0, c["dof"])) for _ in range(batch)]
    return synth.make_ragged_problem(task, c["T"], rows, config_id=config_id, dense_residuals=dense, one_sided_frac=0.1)


def _run(c, p, monkeypatch, kp_ordered=False, pd=100):
    for key in S.ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for key, val in c["env"].items():
        monkeypatch.setenv(key, val)
    fused = bool(c["flags"] & S.FLAG_FUSED)
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], n_alpha=c["n_alpha"], fused=fused,
                tiled=bool(c["flags"] & S.FLAG_TILED)) as e:
        bv = e.backward_variant
        kp_ordered = kp_ordered and bv == "mfma_f64_t1_fused"   # (the key-point ordered payload has no slot for a control beyond dof)
        synth.upload(e, p, kp_ordered=kp_ordered, rx_const=c["rx_const"])
        if not (bv == "mfma_f64_t1_fused" and kp_ordered):      # (the raw fused sweeps difference the payload themselves)
            e.fd_difference()
        if "fused" not in bv:
            e.interpolate()
            if not bv.endswith("_a6"):                           # (a6: the cost derivatives are formed inside the sweeps)
                e.cost_derivs()
        st, dJ = e.backward(p["lam"], pd)
        K, k = e.gains()
        cost, U = e.forward_linear(orc.alphas(c["n_alpha"]), want_U=True)
        return dict(status=st, delta_J=dJ, K=K, k=k, cost=cost, U=U, variants=(bv, e.forward_variant),
                    launch=(e.last_launch("backward"), e.last_launch("forward")))


def _check_dispatch(c, g, n_simd):
    d = S.dispatch(c["dof"], c["m"], c["nr"], c["T"], c["n_alpha"], c["batch"], n_simd, c["flags"], c["env"], c["rx_const"], True,
                   c["uniform"])
    assert g["variants"] == d["variants"], (g["variants"], d)
    for got, want in zip(g["launch"], d["launch"]):
        assert got.startswith(want) if ":" not in want else want in got + ":", (got, want)
    if d["variants"][0] == "mfma_f64_t1_fused":                  # (the key-point set kind the device saw)
        assert all((":uni" in x) == c["uniform"] for x in g["launch"]), g["launch"]
    if d["fwd"][0] == "tiled_fwd":
        assert ":state_cost_waves" not in g["launch"][1], g["launch"]


def _check(g, refs, rows, tag):
    """rows: the trajectories of the GPU result to check; refs[b % len(refs)] is the oracle of trajectory b."""
    for b in rows:
        o = refs[b % len(refs)]
        assert g["status"][b] == o["status"], (tag, b, g["status"][b], o["status"])
        if o["status"] != 0:
            continue
        errs = dict(K=_rel(g["K"][b], o["K"]), k=_rel(g["k"][b], o["k"]),
                    delta_J=abs(g["delta_J"][b] - o["delta_J"]) / max(abs(o["delta_J"]), 1e-300),
                    cost=_rel(g["cost"][b], o["cost_pred"]), U=_rel(g["U"][b], o["U_alpha"]))
        assert max(errs.values()) <= RTOL, (tag, b, g["launch"], errs)


_CASES = [c for c in S.cases(1024) if c["why"] != "refused"]


@pytest.mark.parametrize("c", _CASES, ids=[_case_id(c) for c in _CASES])
def test_shape_matches_oracle(c, monkeypatch):
    n_simd = _n_simd()
    p = _problem(c)
    kp_ordered = bool(c["flags"] & S.FLAG_FUSED) and (c["dof"] + c["nr"]) % 2 == 1     # both payload forms over the fused cases
    g = _run(c, p, monkeypatch, kp_ordered=kp_ordered)
    _check_dispatch(c, g, n_simd)
    refs = [pipeline.run_trajectory(p, b, n_alpha=c["n_alpha"], want_U=True) for b in range(p["batch"])]
    assert all(o["status"] == 0 for o in refs) or c["why"] == "long"
    _check(g, refs, range(p["batch"]), _case_id(c))


def _take(p, batch):
    """The first `batch` trajectories of a problem (job lists filtered, per-trajectory arrays cut)."""
    q = dict(p)
    sel = p["job_b"] < batch
    for key in ("job_b", "job_t", "job_col", "job_mode", "job_nom", "xplus", "xminus"):
        q[key] = p[key][sel]
    for key in ("r", "r_x", "r_u", "u_nom"):
        q[key] = p[key][:batch]
    q["kp_rows"] = p["kp_rows"][:batch]
    q["batch"] = batch
    return q


def test_batch_boundaries(monkeypatch):
    """n_simd and n_simd + 1 trajectories (excl / plain kernels of the one-tile and one-wave fused sweeps), n_simd / 4 and one more
    (the tiled state / cost forward): 7 distinct trajectories tiled, every one of the batch checked against its oracle."""
    n_simd = _n_simd()
    for c in S.batch_cases(n_simd):
        c = dict(c, T=17)
        base = _problem(c, batch=7, config_id=5)
        refs = [pipeline.run_trajectory(base, b, n_alpha=c["n_alpha"], want_U=True) for b in range(7)]
        p = _take(synth.tile_problem(base, -(-c["batch"] // 7)), c["batch"])
        g = _run(c, p, monkeypatch, kp_ordered=bool(c["flags"] & S.FLAG_FUSED))
        _check_dispatch(c, g, n_simd)
        _check(g, refs, range(c["batch"]), _case_id(c))


def test_generic_lds_limit_refused_at_create(monkeypatch):
    """The largest state the generic backward sweep takes with 7 controls runs (test_shape_matches_oracle, dof 46); the next is
    refused by kpilqr_create with KPILQR_ERR_ARG."""
    for key in S.ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    dof = S.GENERIC_MAX_DOF_M7 + 1
    with pytest.raises(KpilqrError) as ei:
        Engine(dof, 7, 5, 4, batch=2)
    assert ei.value.code == -1 and "LDS" in str(ei.value)
