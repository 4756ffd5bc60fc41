"""GPU tests of the FP32 key-point column upload, kpilqr_upload_kp_columns_f32 / kpilqr_upload_kp_columns_f32_partial (columns_f32.hip).

The yardstick of every case is the FP64 call fed the numpy-DECODED doubles (synth.decode_kp_columns_f32: the exact widening, + 1.0 at
the unit rows) on a fresh context of the same flags: the library's decoding must leave the bits that call leaves -- A and B behind
kpilqr_fd_interpolate, and K, k, delta_J, status, cost_pred and U_alpha behind kpilqr_iterate, array_equal.  K and k are also held to
the C oracle run on the decoded columns at the suite's 1e-9.  (What the rounding itself costs is the CPU side:
tests/test_columns_f32_abi.py, tools/columns_f32_error.py.)"""
import functools

import numpy as np
import pytest

import _columns_f32 as cf
from oracle import oracle as orc
from trajoptkp_amd import Engine, host, synth
from trajoptkp_amd.engine import KpilqrError

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -5
ALPHAS = orc.alphas(6)
TIGHT = 1e-9


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


# ---- problems -----------------------------------------------------------------------------------------------------------------
def _by_entry(p):
    """Control columns without a DoF list (m > dof) have no slot in a by-entry payload: dropped, so that the oracle sees the same jobs"""
    keep = p["job_col"] < p["n"] + min(p["m"], p["dof"])
    q = dict(p)
    for k in ("job_b", "job_t", "job_col", "job_mode", "job_nom", "xplus", "xminus"):
        q[k] = p[k][keep]
    return q


def _ragged(task, T, rows, config_id=7):
    return _by_entry(synth.make_ragged_problem(task, T, list(rows), config_id=config_id, one_sided_frac=0.2))


def _bisected(dof, T, seed):
    rng = np.random.default_rng(seed)
    return synth.bisect_keypoints(rng, dof, T, 1, rng.uniform(0.2, 1.0, dof))


def _minimal(dof, T):
    return synth.rows_from_dof_lists(dof, T, [[0, T - 1]] * dof)


@functools.lru_cache(maxsize=None)
def _problem(name):
    if name == "acrobot":            # n = 4, m = 1 < dof: the kind-2 slots of DoF 1 are present and ignored
        return _by_entry(synth.make_problem(task="acrobot", T=37, batch=3, min_N=5, config_id=1, dense_residuals=True, one_sided_frac=0.2))
    if name == "panda_ragged":       # per-DoF lists: ragged entry ranges, an entry count that is no multiple of any block size
        return _ragged("panda_reaching", 64, [_bisected(7, 64, 11), _bisected(7, 64, 12)])
    if name == "pushing":            # n = 20: the tiled family
        return _by_entry(synth.make_problem(task="panda_pushing", T=48, batch=2, min_N=4, config_id=3, dense_residuals=True))
    if name == "m_gt_dof":           # (dof, m, nr) = (3, 5, 3)
        return _by_entry(synth.make_problem(task=synth.shape_task(3, 5, 3), T=33, batch=2, min_N=4, config_id=4, dense_residuals=True))
    if name == "minimal_list":       # one trajectory's lists are the two-entry minimum {0, T-1}
        return _ragged("panda_reaching", 40, [_bisected(7, 40, 21), _minimal(7, 40), _bisected(7, 40, 23)])
    raise KeyError(name)


def _columns(p):
    """(FP64 columns, encoded floats, decoded doubles, DoF of every entry); the ignored kind-2 slots (DoFs >= m) carry a value of their
    own, so that 'ignored' is tested and not assumed"""
    cols = synth.kp_columns(p)
    dofs = synth.kp_entry_dofs(p)
    cols[dofs >= p["m"], 2, :] = 3.25
    c32 = synth.encode_kp_columns_f32(cols, dofs, p["dof"])
    return cols, c32, synth.decode_kp_columns_f32(c32, dofs, p["dof"]), dofs


def _entries_of(p, traj):
    offs, _ = cf.entry_csr(p)
    return np.concatenate([np.arange(offs[b * p["dof"]], offs[(b + 1) * p["dof"]]) for b in traj] + [np.zeros(0, np.int64)]).astype(np.int64)


# ---- contexts -----------------------------------------------------------------------------------------------------------------
def _engine(p, fused):
    e = Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=fused)
    if fused:
        assert "fused" in e.backward_variant
    return e


def _rest(e, p):
    e.upload_residuals(p["r"], p["r_x"], p["r_u"] if np.any(p["r_u"]) else None, p["w_run"], p["w_term"])
    e.upload_nominal(p["u_nom"], p["ctrl_lim"])


def _f64_upload(e, dec, traj=None):
    s = dict(cols=np.ascontiguousarray(dec, np.float64), entries=len(dec))
    e.upload_kp_columns(s) if traj is None else e.upload_kp_columns_partial(traj, s)


def _measure(e, p):
    """A, B behind kpilqr_fd_interpolate; K, k, delta_J, status, cost_pred, U_alpha behind kpilqr_iterate"""
    e.fd_interpolate()
    A, B = e.get_AB()
    e.iterate(p["lam"], 100, ALPHAS)
    res = e.results()
    K, k = e.gains()
    _, U = e.forward_linear(None, want_U=True)             # (the resident alphas: the controls of the iteration's forward sweep)
    return dict(A=A, B=B, K=K, k=k, delta_J=res["delta_J"], status=res["status"], cost_pred=res["cost_pred"], U_alpha=U)


def _same(got, want, what):
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), (what, key)


def _run(p, fused, upload):
    with _engine(p, fused) as e:
        e.set_keypoints_rows(p["kp_rows"])
        upload(e)
        _rest(e, p)
        return _measure(e, p)


def _hold_to_oracle(p, dec, got, what):
    for b in range(p["batch"]):
        o = cf.oracle_on_columns(p, dec, b, p["lam"])
        assert o["status"] == 0 and got["status"][b] == 0
        eK, ek = relerr(got["K"][b], o["K"]), relerr(got["k"][b], o["k"])
        print(f"{what} b={b}: K {eK:.2e} k {ek:.2e} against the oracle on the decoded columns")
        assert eK < TIGHT and ek < TIGHT, (what, b, eK, ek)
        assert relerr(got["A"][b], o["A"]) < 1e-12 and relerr(got["B"][b], o["B"]) < 1e-12


# ---- 1. the decoding leaves the bits of the FP64 call on the decoded doubles ----------------------------------------------------
CASES = [("acrobot", True), ("acrobot", False), ("panda_ragged", True), ("panda_ragged", False), ("pushing", False), ("m_gt_dof", False),
         ("minimal_list", True)]


@pytest.mark.parametrize("name,fused", CASES, ids=[f"{n}-{'fused' if f else 'records'}" for n, f in CASES])
def test_f32_upload_gives_the_bits_of_the_fp64_call_on_the_decoded_columns(name, fused):
    p = _problem(name)
    cols, c32, dec, _ = _columns(p)
    assert np.count_nonzero(dec != cols) > cols.size // 8          # the transport rounds: this is not the FP64 payload again
    want = _run(p, fused, lambda e: _f64_upload(e, dec))
    assert np.all(want["status"] == 0) and np.any(want["K"] != 0)
    got = _run(p, fused, lambda e: e.upload_kp_columns_f32(c32))
    _same(got, want, name)
    _hold_to_oracle(p, dec, got, name)
    if name == "pushing":
        with _engine(p, False) as e:
            assert "tiled" in e.backward_variant


# ---- 2. partial: new lists for a scattered subset, their columns through the partial call ----------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_partial_f32_upload_equals_its_fp64_twin(fused):
    T, B, dof = 40, 5, 7
    rows0 = [_bisected(dof, T, 100 + b) for b in range(B)]
    new = {0: _bisected(dof, T, 900), 2: _minimal(dof, T), 4: synth.rows_from_dof_lists(dof, T, [list(range(T))] * dof)}     # ranges move both ways
    traj = sorted(new)
    p0 = _ragged("panda_reaching", T, rows0)
    p1 = _ragged("panda_reaching", T, [new.get(b, rows0[b]) for b in range(B)])
    for key in ("r", "r_x", "r_u", "u_nom"):                  # (only the lists and the columns change: the rest stays resident)
        p1[key] = p0[key]
    _, c32_0, dec_0, _ = _columns(p0)
    _, c32_1, dec_1, _ = _columns(p1)
    idx = _entries_of(p1, traj)
    kept = [b for b in range(B) if b not in new]
    assert np.array_equal(c32_1[_entries_of(p1, kept)], c32_0[_entries_of(p0, kept)])       # a kept trajectory keeps its columns

    def sequence(e, whole, partial):
        e.set_keypoints_rows(p0["kp_rows"])
        whole(e)
        _rest(e, p0)
        first = _measure(e, p0)
        e.update_keypoints_rows(traj, [new[b] for b in traj])
        partial(e)
        return first, _measure(e, p1)

    def f32_partial(e):
        # rejected first, before anything is enqueued: a list in the wrong order, too few entries, the FP64 call's rules
        for bad_traj, bad in ((traj[::-1], c32_1[idx]), (traj[:-1], c32_1[idx]), (traj, c32_1[idx][:-1])):
            with pytest.raises(KpilqrError) as err:
                e.upload_kp_columns_f32(bad, traj=bad_traj)
            assert err.value.code == ERR_ARG
        e.upload_kp_columns_f32(c32_1[idx], traj=traj)

    with _engine(p0, fused) as e:
        want0, want1 = sequence(e, lambda e: _f64_upload(e, dec_0), lambda e: _f64_upload(e, dec_1[idx], traj))
    with _engine(p0, fused) as e:
        got0, got1 = sequence(e, lambda e: e.upload_kp_columns_f32(c32_0), f32_partial)
    _same(got0, want0, "before the update")
    _same(got1, want1, "after the partial upload")
    for key in ("A", "B", "K", "k", "delta_J", "cost_pred", "U_alpha"):                      # the kept trajectories: unchanged
        assert np.array_equal(got1[key][kept], got0[key][kept]), key
    fresh = _run(p1, fused, lambda e: e.upload_kp_columns_f32(c32_1))                        # ... and all of it is a whole upload's
    _same(got1, fresh, "against a whole upload of the merged lists")
    _hold_to_oracle(p1, dec_1, got1, "partial")


# ---- 3. special values ---------------------------------------------------------------------------------------------------------
def test_special_values_arrive_as_the_decoding_rule_says():
    p = _problem("acrobot")
    dof, n = p["dof"], p["n"]
    _, c32, _, dofs = _columns(p)
    c32 = c32.copy()
    sub = np.float32(1e-40)                                   # an FP32 subnormal
    assert 0 < sub < np.finfo(np.float32).tiny
    specials = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), sub, -sub, np.float32(-0.0)]
    for i, v in enumerate(specials):                          # entry 2i: at the unit rows of both kinds; entry 2i + 1: at ordinary rows
        d = int(dofs[2 * i])
        c32[2 * i, 0, d] = v; c32[2 * i, 1, d + dof] = v
        d = int(dofs[2 * i + 1])
        c32[2 * i + 1, 0, (d + 1) % n] = v; c32[2 * i + 1, 1, d] = v; c32[2 * i + 1, 2, 0] = v
    dec = synth.decode_kp_columns_f32(c32, dofs, dof)
    assert dec[6, 0, int(dofs[6])] == 1.0 and dec[7, 0, (int(dofs[7]) + 1) % n] == np.float64(sub) != 0.0
    offs, times = cf.entry_csr(p)
    with _engine(p, False) as e:
        e.set_keypoints_rows(p["kp_rows"])
        e.upload_kp_columns_f32(c32)
        e.fd_interpolate()
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


# ---- 4. rejections leave everything alone ----------------------------------------------------------------------------------------
def test_rejected_calls_leave_the_payload_and_the_next_iteration_alone():
    p = _problem("panda_ragged")
    _, c32, dec, _ = _columns(p)
    want = _run(p, True, lambda e: e.upload_kp_columns_f32(c32))

    def raises(code, f, *a, **kw):
        with pytest.raises(KpilqrError) as err:
            f(*a, **kw)
        assert err.value.code == code, err.value

    with _engine(p, True) as e:
        raises(ERR_STATE, e.upload_kp_columns_f32, c32)                          # before the key-points it is ordered by
        e.set_keypoints_rows(p["kp_rows"])
        e.upload_kp_columns_f32(c32)
        _rest(e, p)
        raises(ERR_ARG, e.upload_kp_columns_f32, c32[:-1])                       # wrong `entries`
        raises(ERR_ARG, e.upload_kp_columns_f32, np.concatenate([c32, c32[:1]]))
        raises(ERR_ARG, e.upload_kp_columns_f32, c32[:3], traj=[1, 0])           # an unsorted list (and nothing is pending)
        raises(ERR_ARG, e.upload_kp_columns_f32, c32[:3], traj=[0])
        assert e._L.kpilqr_upload_kp_columns_f32(e._h, None, len(c32)) == ERR_ARG
        _same(_measure(e, p), want, "after the rejected calls")


# ---- 5. the FP64 path is untouched by a context's FP32 history --------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_fp64_columns_after_an_f32_upload_give_a_fresh_context_s_bits(fused):
    p = _problem("panda_ragged")
    cols, c32, _, _ = _columns(p)
    want = _run(p, fused, lambda e: _f64_upload(e, cols))

    def both(e):
        e.upload_kp_columns_f32(c32)
        _f64_upload(e, cols)
    got = _run(p, fused, both)
    _same(got, want, "FP64 after FP32")
    assert not np.array_equal(got["K"], _run(p, fused, lambda e: e.upload_kp_columns_f32(c32))["K"])      # (and the FP32 payload is another one)


# ---- 6. the host class --------------------------------------------------------------------------------------------------------------
def test_host_class_f32_columns_equal_the_run_on_the_decoded_doubles():
    kw = dict(T=100, min_N=5, max_iter=6, min_iter=2, torque_weight=1e-3)
    f64 = host.run_acrobot(method="set_interval+fused+columns", **kw)
    twin = host.run_acrobot(method="set_interval+fused+columns+hostf32cols", **kw)       # rounded alike, decoded on the host, uploaded as FP64
    f32 = host.run_acrobot(method="set_interval+fused+columns+f32cols", **kw)
    assert f32["iterations"] == twin["iterations"] and f32["iterations"] >= 2
    assert np.array_equal(f32["cost_history"], twin["cost_history"]) and np.array_equal(f32["U"], twin["U"])
    assert np.array_equal(f32["K0"], twin["K0"])
    assert f32["cost_history"][-1] < f32["cost_history"][0]
    # half the bytes of the FP64-column run with as many linearisations (the twin: the same decisions by construction)
    assert twin["payload_bytes_uploaded"] > 0 and 2 * f32["payload_bytes_uploaded"] == twin["payload_bytes_uploaded"]
    if f64["iterations"] == f32["iterations"]:
        assert 2 * f32["payload_bytes_uploaded"] == f64["payload_bytes_uploaded"]
