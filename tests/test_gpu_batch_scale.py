"""The kernels AROUND the sweeps at list and trajectory counts beyond one workgroup, on batches whose members all differ
(tests/_batch_scale.py builds the problems and says what it asserts of them; tests/test_batch_scale_inputs.py checks them on the CPU).

  1a  k_kp_flags / k_kp_scan / k_kp_fill: device placement against the oracle's at 1022 .. 2051 lists (k_kp_scan sums
      per = ceil(lists / 1024) counts a thread above 1024 lists), array_equal, and the count the library read back
  1b  the lists the device placed drive a whole iteration (entry tables, segment map / segent, interpolation) on a fused context and on
      one with step records, every trajectory against the oracle
  1c  the device's uniform flag (k_kp_uniform) with ONE list that differs, in the first, a middle and the last block, and beyond the
      256-thread stride inside a list
  2   both sides of every batch bound of _shapes.batch_cases with B distinct trajectories, the consumer / helper pair at #SIMDs / 2,
      and the paired forward scoring with eight alphas above #SIMDs
  3   listed calls with long scattered lists on fused Panda contexts of #SIMDs + 1 trajectories: regeneration, the gain downloads of a
      list, the streamed upload of a list (k_rows_in, k_rows_in_entries, the ring of staged lists)

Bars: placement array_equal; 1e-9 relative against oracle.pipeline.run_trajectory for K, k, delta_J, cost_pred (and U_alpha in section
2), status exact; A and B of a context with records array_equal; listed calls bit for bit against a fresh context.

Dropped shape: (dof 64, B 17) of the placement table -- kpilqr_create refuses a generic context of 64 DoFs (the LDS bound of its
backward sweep), so no context exists to place its lists on."""
import ctypes as C

import numpy as np
import pytest

import _batch_scale as BS
import _shape_run as R
import _shapes as S
from _sequences import _entries_of
from oracle import oracle as orc
from oracle import pipeline
from trajoptkp_amd import Engine, _lib, synth
from trajoptkp_amd.engine import KpilqrError, rows_to_dof_csr

pytestmark = pytest.mark.gpu

ERR_ARG = -1
NO_ENV = {"env": {}}


def _result(e):
    K, k = e.gains()
    res = e.results()
    return dict(status=res["status"], K=K, k=k, delta_J=res["delta_J"], cost=res["cost_pred"])


# ---- 1a. placement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", BS.KP_HORIZONS)
@pytest.mark.parametrize("dof,B", BS.KP_SHAPES, ids=[f"d{d}b{b}" for d, b in BS.KP_SHAPES])
def test_device_placement_matches_oracle_beyond_1024_lists(dof, B, T):
    """All four methods on one context.  offsets and times array_equal the oracle's through rows_to_dof_csr; offsets[-1] is the number
    of times; and the count the library read back from the device is that number: a key-point ordered payload of exactly so many
    entries is accepted, one of an entry less is refused."""
    kw = BS.kp_context(dof)
    with Engine(dof, kw["m"], T, kw["nr"], batch=B, generic=kw["generic"]) as e:
        e.upload_states(BS.kp_states(dof, B, T))
        for method in BS.KP_METHODS:
            min_N, max_N, thr = BS.kp_params(method, dof, T)
            o_ref, t_ref = BS.kp_reference(method, dof, B, T)
            e.generate_keypoints(method, min_N, max_N, thr, BS.KP_DT)
            o_dev, t_dev = e.get_keypoints()
            assert np.array_equal(o_dev, o_ref), (method, dof, B, T, np.flatnonzero(o_dev != o_ref)[:4])
            assert np.array_equal(t_dev, t_ref), (method, dof, B, T)
            total = int(o_ref[-1])
            assert o_dev[-1] == len(t_dev) == total
            lay = _lib.FdkpLayout()
            e._ck(e._L.kpilqr_fd_kp_layout(e._h, total, C.byref(lay)))
            slab = np.zeros(max(lay.bytes, 1), np.uint8)                 # (zeros: only the count is under test)
            with pytest.raises(KpilqrError) as ei:
                e.upload_fd_kp(dict(slab=slab, entries=total - 1))
            assert ei.value.code == ERR_ARG, (method, str(ei.value))
            e.upload_fd_kp(dict(slab=slab, entries=total))
            e.sync()


# ---- 1b. the placed lists drive an iteration ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", list(BS.FEED_METHODS))
@pytest.mark.parametrize("dof,B", list(BS.FEED_SHAPES), ids=[f"d{d}b{b}" for d, b in BS.FEED_SHAPES])
def test_device_placed_lists_drive_an_iteration(dof, B, method, monkeypatch):
    R._set_env(NO_ENV, monkeypatch)
    p, X, min_N, max_N, thr = BS.feed_problem(dof, B, method)
    refs = BS.references(p)
    BS.distinct(p, refs)
    want_o, want_t = rows_to_dof_csr(p["kp_rows"], dof, p["T"])
    for fused in (True, False):
        with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=B, fused=fused) as e:
            assert ("fused" in e.backward_variant) == fused, e.backward_variant
            synth.upload(e, p, keypoints=False)
            e.upload_states(X)
            e.generate_keypoints(method, min_N, max_N, thr, BS.KP_DT)
            e.iterate(p["lam"], 100, BS.ALPHAS)
            got = _result(e)
            o, t = e.get_keypoints()
            if not fused:
                A, Bm = e.get_AB()
        assert np.array_equal(o, want_o) and np.array_equal(t, want_t)
        BS.hold(got, refs, range(B), (dof, B, method, fused))
        if not fused:
            for b in range(B):
                assert np.array_equal(A[b], refs[b]["A"]) and np.array_equal(Bm[b], refs[b]["B"]), (dof, B, method, b)


# ---- 1c. the uniform flag ----------------------------------------------------------------------------------------------------------------
def _uniform_run(p, uniform, tag):
    refs = BS.references(p)
    BS.distinct(p, refs)
    with Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=True) as e:
        synth.upload(e, p, kp_ordered=True, rx_const=True)
        e.iterate(p["lam"], 100, BS.ALPHAS)
        got = _result(e)
        launch = (e.last_launch("backward"), e.last_launch("forward"))
    assert (":uni" in launch[1]) == uniform and (":uni" in launch[0]) == uniform, (tag, launch)
    BS.hold(got, refs, range(p["batch"]), tag)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_odd_list_clears_the_uniform_flag(where, monkeypatch):
    """#SIMDs + 1 Panda trajectories on set_interval lists; the last DoF of ONE trajectory has a key-point more.  The flag is cleared
    by whichever workgroup of k_kp_uniform finds the difference: the first, a middle one, the last."""
    R._set_env(NO_ENV, monkeypatch)
    B = R._n_simd() + 1
    odd = {"first": 0, "middle": B // 2, "last": B - 1}[where]
    _uniform_run(BS.uniform_problem(B, odd), False, ("odd", odd))
    _uniform_run(BS.uniform_problem(B, None), True, ("nobody", where))


def test_a_difference_beyond_the_stride_inside_a_list_clears_the_uniform_flag(monkeypatch):
    """T = 300, B = 3, lists of 299 entries (every step but one: tests/_batch_scale.py, long_uniform_problem, says why not 300): the
    last DoF of trajectory 2 differs from the others at list index 290 alone, which only the second round of the 256 threads of
    k_kp_uniform looks at."""
    R._set_env(NO_ENV, monkeypatch)
    _uniform_run(BS.long_uniform_problem(True), False, "long, odd")
    _uniform_run(BS.long_uniform_problem(False), True, "long, nobody")


# ---- 2. both sides of every batch bound -----------------------------------------------------------------------------------------------
_BOUND_IDS = [R._case_id(c) for c in BS.bound_cases(BS.N_SIMD)]


@pytest.mark.parametrize("i", range(len(_BOUND_IDS)), ids=_BOUND_IDS)
def test_distinct_trajectories_on_both_sides_of_the_batch_bounds(i, monkeypatch):
    n_simd = R._n_simd()
    c = BS.bound_cases(n_simd)[i]
    p = BS.bound_problem(c)
    refs = BS.references(p, c["n_alpha"])
    BS.distinct(p, refs)
    R._set_env(c, monkeypatch)
    with R._engine(c, p) as e:
        st, dJ = R._backward(e, c, p, kp_ordered=bool(c["flags"] & S.FLAG_FUSED))
        K, k = e.gains()
        cost, U = e.forward_linear(orc.alphas(c["n_alpha"]), want_U=True)
        g = dict(status=st, delta_J=dJ, K=K, k=k, cost=cost, U=U, **R._launched(e))
        scoring = e.last_launch("forward_scoring")
    R._check_dispatch(c, g, n_simd)
    if c["why"] == "alpha8":
        assert scoring == "pair2" and g["launch"][1].endswith(":w1:uni:ru0:rxc"), (scoring, g["launch"])
    R._check(g, refs, range(p["batch"]), R._case_id(c))


# ---- 3. listed calls with long, scattered lists -------------------------------------------------------------------------------------------
LISTS = ("third", "half", "all_but_one")


def _listed_engine(p):
    e = Engine(p["dof"], p["m"], p["T"], p["nr"], batch=p["batch"], fused=True)
    assert e.backward_variant == "mfma_f64_t1_fused"
    e.set_lambda_retry()                       # (the schedule never fires here: lambda_retry() then reports every trajectory's lambda and one attempt)
    return e


def _whole(e, p, lam):
    e.set_keypoints_rows(p["kp_rows"])
    e.upload_fd_kp(e.fd_kp_slab(*synth.kp_ordered_payload(p)), eps=p["eps"])
    e.upload_residuals(p["r"], p["r_x"], p["r_u"], p["w_run"], p["w_term"])
    e.upload_nominal(p["u_nom"], p["ctrl_lim"])
    e.iterate(lam, 100, BS.ALPHAS)


def _snapshot(e):
    out = _result(e)
    out["lam"], out["attempts"] = e.lambda_retry()
    return out


@pytest.mark.parametrize("name", LISTS)
def test_regeneration_of_a_long_list(name, monkeypatch):
    """One context: the whole batch, then new ragged lists, payload, residuals and nominal controls for the listed trajectories and
    kpilqr_iterate_partial at new lambdas.  Listed rows: the bits of a fresh context that is given exactly those trajectories' final
    inputs (the contract of tests/test_gpu_partial_sweeps.py: the form of a listed launch follows the count, as a context of that many
    trajectories chooses it) and the oracle at 1e-9; every other row of K, k, status, delta_J, cost_pred, lambda and attempts: the
    bits it had before."""
    R._set_env(NO_ENV, monkeypatch)
    B = R._n_simd() + 1
    who = BS.listed_lists(B)[name]
    rest = np.setdiff1d(np.arange(B), who)
    p0, p1 = BS.listed_base(B), BS.listed_regenerated(B, name)
    lam0, lam1 = BS.listed_lambdas(B, 0), BS.listed_lambdas(B, 1)
    with _listed_engine(p0) as e:
        _whole(e, p0, lam0)
        snap = _snapshot(e)
        e.update_keypoints_rows(who, [p1["kp_rows"][b] for b in who])
        xp, xm, md = synth.kp_ordered_payload(p1)
        idx = _entries_of(p1, who)
        e.upload_fd_kp_partial(who, e.fd_kp_slab(xp[idx], xm[idx], md[idx]), eps=p1["eps"])
        e.upload_residuals_partial(who, p1["r"][who], p1["r_x"][who], p1["r_u"][who])
        e.upload_nominal_partial(who, p1["u_nom"][who])
        e.iterate_partial(who, lam1[who], 100, BS.ALPHAS)
        after = _snapshot(e)
        launch = (e.last_launch("backward"), e.last_launch("forward"))
        o, t = e.get_keypoints()
    assert all(x.endswith(":subset") for x in launch), launch
    wo, wt = rows_to_dof_csr(p1["kp_rows"], p1["dof"], p1["T"])
    assert np.array_equal(o, wo) and np.array_equal(t, wt)
    assert not np.any(snap["status"]) and np.all(snap["attempts"] == 1) and np.array_equal(snap["lam"], lam0)
    for key in snap:                                               # nobody else's bytes
        assert np.array_equal(after[key][rest], snap[key][rest]), (name, key, "unlisted rows changed")
    assert not np.array_equal(after["K"][who], snap["K"][who])
    q = BS.sub(p1, who)
    with _listed_engine(q) as f:
        _whole(f, q, lam1[who])
        fresh = _snapshot(f)
    for key in fresh:                                              # the bits of the fresh context
        assert np.array_equal(after[key][who], fresh[key]), (name, key, np.flatnonzero([not np.array_equal(a, b) for a, b in zip(after[key][who], fresh[key])])[:8])
    refs = {b: pipeline.run_trajectory(p1, b, lam=float(lam1[b]), want_U=True) for b in who}
    BS.hold(after, refs, who, name)


def test_gain_downloads_of_long_lists(monkeypatch):
    """gains(traj=list), FP64 and FP32, are the rows of the whole downloads (k_gains_out, k_gains_f32 with a list); the whole FP64
    download is held to the oracle, so the rows are the right ones and not merely the same ones."""
    R._set_env(NO_ENV, monkeypatch)
    B = R._n_simd() + 1
    p0, lam0 = BS.listed_base(B), BS.listed_lambdas(B, 0)
    refs = BS.references(p0, lam=lam0)
    BS.distinct(p0, refs)
    with _listed_engine(p0) as e:
        _whole(e, p0, lam0)
        whole = _result(e)
        K32, k32 = e.gains(f32=True)
        assert K32.dtype == np.float32 and np.array_equal(k32, whole["k"])
        for name in LISTS:
            who = BS.listed_lists(B)[name]
            K, k = e.gains(traj=who)
            assert np.array_equal(K, whole["K"][who]) and np.array_equal(k, whole["k"][who]), name
            Kf, kf = e.gains(traj=who, f32=True)
            assert Kf.dtype == np.float32 and np.array_equal(Kf, K32[who]) and np.array_equal(kf, whole["k"][who]), name
    BS.hold(whole, refs, range(B), "whole")
    with np.errstate(over="ignore", under="ignore"):
        assert np.array_equal(K32, whole["K"].astype(np.float32))


def test_streamed_uploads_of_long_lists(monkeypatch):
    """kpilqr_iterate_streamed4 with upload_traj on one long-lived context: at 1, 3 and 4 chunks a whole call, then four calls in a row
    with four different long lists, each bringing other data (rows and key-point ordered records) for its trajectories -- no wait in
    between, and the ring of four staged lists goes round three times.  The outputs of call i are the bits of
    kpilqr_iterate_streamed3 on a fresh context given whole-batch arrays with the data of calls 0 .. i mixed in (the yardstick of
    tests/test_gpu_streamed_subset.py)."""
    import _streamed_subset as ss
    R._set_env(NO_ENV, monkeypatch)
    B = R._n_simd() + 1
    p, kind = BS.listed_base(B), "fd_kp"
    lists = list(BS.listed_lists(B).values())
    assert len(lists) == 4
    rowsA, payA = ss.rows_of(p, "A"), ss.payload_of("batch_scale", p, kind, "A")

    def rows_i(i):
        out = dict(rowsA)
        out["r"] = rowsA["r"] * (1.0 + 0.01 * (i + 1)) + 0.003
        out["r_x"] = rowsA["r_x"] * (1.0 - 0.02 * (i + 1))
        out["u_nom"] = rowsA["u_nom"] * (1.0 - 0.03 * (i + 1)) + 0.01
        return out

    def pay_i(i):
        xp, xm, mode = payA
        return (xm + (0.9 - 0.1 * i) * (xp - xm), xm, mode)

    refs = []
    with ss.Yardstick("batch_scale", True, kind, p=p) as yard:
        rows, pay = dict((k, v.copy()) for k, v in rowsA.items()), payA
        for i, who in enumerate(lists):
            new = rows_i(i)
            for key in rows:
                rows[key][who] = new[key][who]
            pay = ss.mix(pay, pay_i(i), ss.entry_index(p, who))
            refs.append(yard.run(rows, pay))
    assert all(not np.any(r["status"]) for r in refs) and not ss.same(refs[0]["K"], refs[1]["K"]) and not ss.same(refs[2]["K"], refs[3]["K"])
    # the yardstick's last mixture against the oracle on the same rows and on the columns of the mixed records: the yardstick runs
    # whole-batch kernels of this library too
    xp, xm, mode = pay
    den = np.where((mode.astype(np.int32)[:, None] >> np.arange(3)[None, :]) & 1, float(p["eps"]), 2.0 * float(p["eps"]))
    oracle = BS.references_on_columns(p, rows, (xp - xm) / den[:, :, None], np.full(B, p["lam"]))
    last = dict(refs[-1], cost=refs[-1]["cost_pred"])
    BS.hold(last, oracle, range(B), "the last mixture")
    with ss.engine(p, True) as e:
        ss.setup(e, p)
        lam = ss.lam_of(e, p)
        whole = dict(ss.pin_rows(e, rowsA), **ss.pin_payload(e, kind, payA))
        ins = [dict(ss.pin_payload(e, kind, ss.take(pay_i(i), ss.entry_index(p, who))), **ss.pin_rows(e, rows_i(i), who)) for i, who in enumerate(lists)]
        first, outs = ss.Outputs(e), [ss.Outputs(e) for _ in lists]
        for nchunks in (1, 3, 4):
            ss.call(e, first, nchunks, lam, p["eps"], **whole)
            for i, who in enumerate(lists):
                ss.call(e, outs[i], nchunks, lam, p["eps"], upload_traj=who, **ins[i])
            e.sync()
            for i in range(len(lists)):
                ss.check(outs[i], refs[i], what=(nchunks, i))
            assert ss.launches(e) == refs[-1]["launch"], (nchunks, ss.launches(e), refs[-1]["launch"])
