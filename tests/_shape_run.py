"""What tests/test_gpu_shapes.py and tests/test_gpu_clamp.py share: the problem of a case of tests/_shapes.py, its run through
the C ABI -- FD, interpolation, cost, backward, forward over the alphas --, the assertion of the variant and launch strings the
table predicts, and the comparison with oracle.pipeline.run_trajectory."""
import numpy as np

import _blockwise as BW
import _shapes as S
from oracle import oracle as orc
from trajoptkp_amd import Engine, synth

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


def _problem(c, batch=None, config_id=4, min_N=4):
    task = synth.shape_task(c["dof"], c["m"], c["nr"])
    batch = c["batch"] if batch is None else batch
    dense = False if c["rx_const"] else True
    if c["uniform"]:
        return synth.make_problem(task=task, T=c["T"], batch=batch, min_N=min_N, dense_residuals=dense, one_sided_frac=0.1,
                                  config_id=config_id)
    # per-DoF lists that differ whatever the seed: DoF 0 has key-points at the ends only, the last one splits every interval
    rng = np.random.default_rng(1000 * c["dof"] + c["m"])
    rows = [synth.bisect_keypoints(rng, c["dof"], c["T"], 2, np.linspace(0.0, 1.0, c["dof"])) for _ in range(batch)]
    return synth.make_ragged_problem(task, c["T"], rows, config_id=config_id, dense_residuals=dense, one_sided_frac=0.1)


def _set_env(c, monkeypatch):
    for key in S.ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for key, val in c["env"].items():
        monkeypatch.setenv(key, val)


def _engine(c, p):
    """The context of case c for problem p (the environment of the case is read at creation: _set_env first)."""
    return Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], n_alpha=c["n_alpha"], fused=bool(c["flags"] & S.FLAG_FUSED),
                  tiled=bool(c["flags"] & S.FLAG_TILED), generic=bool(c["flags"] & S.FLAG_GENERIC))


def _backward(e, c, p, kp_ordered=False, pd=100):
    """Upload, the stages the context's family needs, and the backward sweep: (status, delta_J)."""
    bv = e.backward_variant
    kp_ordered = kp_ordered and bv == "mfma_f64_t1_fused"   # (the key-point ordered payload has no slot for a control beyond dof)
    synth.upload(e, p, kp_ordered=kp_ordered, rx_const=c["rx_const"])
    if not (bv == "mfma_f64_t1_fused" and kp_ordered):      # (the raw fused sweeps difference the payload themselves)
        e.fd_difference()
    if "fused" not in bv:
        e.interpolate()
        if not bv.endswith("_a6"):                           # (a6: the cost derivatives are formed inside the sweeps)
            e.cost_derivs()
    return e.backward(p["lam"], pd)


def _launched(e):
    return dict(variants=(e.backward_variant, e.forward_variant), launch=(e.last_launch("backward"), e.last_launch("forward")))


def _run(c, p, monkeypatch, kp_ordered=False, pd=100):
    _set_env(c, monkeypatch)
    with _engine(c, p) as e:
        st, dJ = _backward(e, c, p, kp_ordered, pd)
        K, k = e.gains()
        cost, U = e.forward_linear(orc.alphas(c["n_alpha"]), want_U=True)
        return dict(status=st, delta_J=dJ, K=K, k=k, cost=cost, U=U, **_launched(e))


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


def _errs(g, o, b, p=None, ref_b=None, n_alpha=6, pd=100):
    """Relative errors of trajectory b of a GPU result against its oracle o (the largest error over the largest entry).  With the
    problem p whose trajectory ref_b (default b) the oracle o is: also `blockwise`, the families of tests/_blockwise.py that are over
    their bar against the extended reference -- [] where every block of K, k, U_alpha and the predicted costs is within it."""
    out = _global_errs(g, o, b)
    if p is not None:
        bb = BW.bars(p, b if ref_b is None else ref_b, n_alpha=n_alpha, pd_stride=pd)
        out["blockwise"] = BW.violations(BW.block_errors(BW.gpu_result(g, b), bb["ref"]), bb["bar"])
    return out


def _global_errs(g, o, b):
    return dict(K=_rel(g["K"][b], o["K"]), k=_rel(g["k"][b], o["k"]),
                delta_J=abs(g["delta_J"][b] - o["delta_J"]) / max(abs(o["delta_J"]), 1e-300),
                cost=_rel(g["cost"][b], o["cost_pred"]), U=_rel(g["U"][b], o["U_alpha"]))


def _check(g, refs, rows, tag, p=None, n_alpha=6):
    """rows: the trajectories of the GPU result to check; refs[b % len(refs)] is the oracle of trajectory b.  p: the problem whose
    trajectories the refs are, in their order -- with it every block is held to its bar as well (_errs)."""
    for b in rows:
        o = refs[b % len(refs)]
        assert g["status"][b] == o["status"], (tag, b, g["status"][b], o["status"])
        if o["status"] != 0:
            continue
        errs = _errs(g, o, b, p, b % len(refs), n_alpha)
        blockwise = errs.pop("blockwise", [])
        assert max(errs.values()) <= RTOL, (tag, b, g["launch"], errs)
        assert not blockwise, (tag, b, g["launch"], blockwise)


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
