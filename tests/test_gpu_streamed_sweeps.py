"""GPU tests of kpilqr_iterate_streamed5: the chunk pipeline linearising and sweeping a LISTED subset of the batch -- per chunk the
listed launches of kpilqr_iterate_partial on the chunk's slice of the list, the compact lambdas placed by k_rows_in, the compact
small outputs gathered by k_rows_out straight into the caller's pinned rows.

The yardstick is never the code under test: the explicit route (kpilqr_update_keypoints, the _partial uploads, kpilqr_iterate_partial)
on a second context that starts from the same resident state, tests/_streamed_sweeps.py.  Those are the same kernels on the same
device bytes with the wave forms forced, so every compact output and every listed row of the device buffers must be its bits, and every
unlisted row the bits of the snapshot taken before the call.  Listed trajectories are also held to the C oracle at the suite's 1e-9.

Shapes, contexts and sentinel-guarded outputs are those of tests/test_gpu_streamed_columns_f32.py (panda7, acrobot3, panda5rec,
pushing3, ragged5 fused and with records).  With three chunks the batches are cut [0,2) [2,4) [4,7) | [0,1) [1,3) [3,5) | one each.
On the CPU oracle no trajectory of these data sets fails at its own lambda (tests/test_gpu_streamed_subset.py holds the same mixtures);
the lambda of an unlisted trajectory has no read-back without a retry schedule and is held in test_lambda_retry."""
import ctypes as C

import numpy as np
import pytest

import _columns_f32 as cf
import _streamed_subset as ss
import _streamed_sweeps as sw
from _streamed_sweeps import CONTEXTS, IDS, KINDS, Outputs, SWEEP_LISTS, problem, same
from test_gpu_streamed_columns_f32 import ragged_rows
from trajoptkp_amd import _lib

pytestmark = pytest.mark.gpu


def mixed(p, name, kind, upload):
    """data set A with B's rows and payload entries for `upload`: what the device holds after the uploads"""
    rows, rb = ss.rows_of(p, "A"), ss.rows_of(p, "B")
    idx = np.asarray(upload, np.int64)
    for k in rows:
        rows[k][idx] = rb[k][idx]
    pay = ss.mix(ss.payload_of(name, p, kind, "A"), ss.payload_of(name, p, kind, "B"), ss.entry_index(p, upload))
    return rows, pay


def full(after):
    return dict(K=after["K"], k=after["k"], status=after["status"])


# ---- 1. a subset equals the explicit route, and nobody else is written -----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,fused", CONTEXTS, ids=IDS)
def test_subset_equals_the_explicit_route(name, fused, kind, monkeypatch):
    p = problem(name)
    B = p["batch"]
    held = 0
    for form in sw.forms_of(name, fused):
        sw.set_form(monkeypatch, form)
        with ss.engine(p, fused) as e, ss.engine(p, fused) as y:
            ss.setup(e, p); ss.setup(y, p)
            # (sweep list, upload list, chunk counts): everything at every chunk count with upload = sweep; a proper subset uploaded,
            # the rest of the list swept again at a lambda of its own, at three chunks
            cases = [(s, s, sw.chunk_counts(B)) for s in SWEEP_LISTS[B]]
            cases += [(s, s[1:], [3]) for s in SWEEP_LISTS[B][2:5]] + [(s, [], [2]) for s in SWEEP_LISTS[B][3:4]]
            for sweep, upload, counts in cases:
                lam = sw.lam_for(p, sweep, distinct=upload != sweep)
                sw.whole(y, p, name, kind, five=False)
                want = sw.explicit(y, p, name, kind, sweep, upload, lam)
                want_launch = sw.launches(y)
                assert np.all(want["status"][sweep] == 0)
                gain = sweep if sweep else [0, B - 1]            # (nobody swept: gains still come down)
                for nchunks in counts:
                    what = (form, sweep, upload, nchunks)
                    sw.whole(e, p, name, kind, nchunks)
                    snap = sw.buffers(e)
                    out, after = sw.streamed(e, p, name, kind, sweep, upload, lam, nchunks, gain=gain)
                    sw.check_compact(out, sweep, gain, want, what=what)
                    sw.check_buffers(after, snap, want, sweep, what=what)
                    if sweep:
                        sw.check_launches(e, form, want_launch)
                        assert not same(after["K"][sweep], snap["K"][sweep]), what
                    else:
                        assert not any(x.endswith(":subset") for x in sw.launches(e)), sw.launches(e)
                # the C oracle, where the whole batch is one consistent problem: upload = sweep at the problem's own lambda
                if kind != "fd_kp" and sweep == SWEEP_LISTS[B][2] and upload == sweep:
                    rows, pay = mixed(p, name, kind, upload)
                    cols = ss.decoded_columns(name, p, kind, pay)
                    assert cf.oracle_on_columns(dict(p, **rows), cols, sweep[0], p["lam"])["status"] == 0      # a listed trajectory is held
                    held += ss.hold_to_oracle(p, rows, cols, full(after), f"{name} fused={fused} {kind} {form} {sweep}")
    assert kind == "fd_kp" or held > 0


# ---- 2. sweep_traj = NULL is kpilqr_iterate_streamed4 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("panda7", True), ("panda5rec", False)])
def test_null_list_is_streamed4(name, fused):
    p = problem(name)
    got = {}
    for five in (False, True):
        with ss.engine(p, fused) as e:
            ss.setup(e, p)
            lam = ss.lam_of(e, p)
            sw.whole(e, p, name, "cols", five=five)
            for i, (kind, gain, f32, up) in enumerate((("cols", None, False, [1, 3]), ("cols", [1, 2], True, None), ("cols", None, False, []))):
                out = Outputs(e)
                kw = {} if not up else sw.listed_inputs(e, p, name, kind, up)
                if five:
                    sw.call5(e, out, 3, lam, p["eps"], upload=up, gain=gain, f32=f32, **kw)
                else:
                    ss.call(e, out, 3, lam, p["eps"], upload_traj=up, gain=gain, f32=f32, **kw)
                e.sync()
                count = None if gain is None else len(gain)
                res = dict((n, out.rows(n).copy()) for n in ("cost_pred", "delta_J", "status"))
                res["K"] = out.rows("K32" if f32 else "K", count).copy()
                res["k"] = out.rows("k", count).copy()
                res["launch"] = sw.launches(e)
                got[five, i] = res
    for i in range(3):
        old, new = got[False, i], got[True, i]
        assert old["launch"] == new["launch"] and not any(":subset" in x for x in new["launch"]), new["launch"]
        for key in ss.OUT:
            assert same(new[key], old[key]), (i, key)
    assert np.all(got[False, 0]["status"] == 0) and np.any(got[False, 0]["K"] != 0)


# ---- 3. the library's own choice of forms: a slice on a chunk's share of the SIMDs ---------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("panda7", True), ("panda5rec", False)])
def test_unforced_forms(name, fused, monkeypatch):
    for key in ("KPILQR_FUSED_WAVES", "KPILQR_FUSED_FWD_WAVES"):
        monkeypatch.delenv(key, raising=False)
    p, kind = problem(name), "cols"
    sweep = SWEEP_LISTS[p["batch"]][3]
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        for nchunks in (1, 3):
            sw.whole(e, p, name, kind, nchunks)
            snap = sw.buffers(e)
            out, after = sw.streamed(e, p, name, kind, sweep, sweep, sw.lam_for(p, sweep, False), nchunks, gain=sweep)
            sw.check_buffers(after, snap, after, sweep, what=nchunks)          # (unlisted bytes; the listed rows are held below)
            sw.check_compact(out, sweep, sweep, after, what=nchunks)
            rows, pay = mixed(p, name, kind, sweep)
            assert cf.oracle_on_columns(dict(p, **rows), pay[0], sweep[0], p["lam"])["status"] == 0
            assert ss.hold_to_oracle(p, rows, pay[0], full(after), f"{name} unforced {nchunks}") >= len(sweep)
            assert all(x.endswith(":subset") for x in sw.launches(e)), sw.launches(e)


# ---- 4. calls in flight with different sweep lists ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("panda7", True), ("panda5rec", False), ("ragged5", True)])
def test_calls_in_flight_with_different_sweep_lists(name, fused, monkeypatch):
    """Three calls enqueued before ONE wait, each with its own sweep list, lambdas and output buffers; then five in a row, so a slot of
    the ring of lists is used again."""
    sw.set_form(monkeypatch, "one_wave")
    p, kind = problem(name), "cols"
    B = p["batch"]
    L = SWEEP_LISTS[B]
    plan = [(L[2], L[2]), (L[1], []), (L[4], [])] + [(L[i % 2 + 2], []) for i in range(5)]
    lams = [sw.lam_for(p, s, True) * (1.0 + 0.1 * i) for i, (s, _) in enumerate(plan)]
    with ss.engine(p, fused) as y:
        ss.setup(y, p)
        sw.whole(y, p, name, kind, five=False)
        wants = [sw.explicit(y, p, name, kind, s, u, lam) for (s, u), lam in zip(plan, lams)]
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        sw.whole(e, p, name, kind)
        ins = [sw.listed_inputs(e, p, name, kind, u) for _, u in plan]
        pl = [sw.pinned_lam(e, lam) for lam in lams]
        outs = [Outputs(e) for _ in plan]
        for first, last in ((0, 3), (3, 8)):
            for i in range(first, last):
                s, u = plan[i]
                sw.call5(e, outs[i], 3, pl[i], p["eps"], sweep=s, upload=u if u else None, gain=s, **ins[i])
            e.sync()
            for i in range(first, last):
                sw.check_compact(outs[i], plan[i][0], plan[i][0], wants[i], what=("in flight", i))
        after = sw.buffers(e)
        for key in sw.BUFS:
            assert same(after[key], wants[-1][key]), key
    assert not same(wants[0]["K"], wants[2]["K"]) and not same(wants[3]["K"], wants[4]["K"])


# ---- 5. a chunk with nobody listed, and sweep_count = 0 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("panda7", True), ("pushing3", False)])
def test_empty_chunks_and_empty_list(name, fused):
    p, kind = problem(name), "cols"
    B = p["batch"]
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        sw.whole(e, p, name, kind)
        snap = sw.buffers(e)
        before = sw.launches(e)
        gain = [0, B - 1]
        for f32 in (False, True):
            out, after = sw.streamed(e, p, name, kind, [], [], np.zeros(0), B, gain=gain, f32=f32)       # one chunk per trajectory, nobody listed
            sw.check_compact(out, [], gain, snap, f32=f32, what="sweep_count = 0")
            out.untouched("cost_pred", "delta_J", "status")
            for key in sw.BUFS:
                assert same(after[key], snap[key]), key
            assert sw.launches(e) == before
        # the last trajectory alone, one chunk each: every other chunk launches nothing but its share of the gain download
        lam = sw.lam_for(p, [B - 1], True)
        with ss.engine(p, fused) as y:
            ss.setup(y, p)
            sw.whole(y, p, name, kind, five=False)
            want = sw.explicit(y, p, name, kind, [B - 1], [], lam)
        out, after = sw.streamed(e, p, name, kind, [B - 1], [], lam, B, gain=gain)
        sw.check_compact(out, [B - 1], gain, want, what="last alone")
        sw.check_buffers(after, snap, want, [B - 1], what="last alone")


# ---- 6. changed key-points --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_changed_keypoints(fused, kind, monkeypatch):
    """ragged5: trajectories {0, 4} get new lists (0: a key-point at every step; 4: its own list again); the call uploads {0, 4} and
    sweeps {0, 2, 4}.  Before it, a call that leaves the payload of a pending trajectory out is refused and changes nothing."""
    sw.set_form(monkeypatch, "one_wave")
    name, more, up, sweep = "ragged5", (0, 4), [0, 4], [0, 2, 4]
    p, p2 = problem(name), problem(name, True, more)
    rows = ragged_rows(more)
    new_rows = {0: rows[0], 4: rows[4]}
    payB = ss.payload_of(name, p2, kind, "B", more)
    lam = sw.lam_for(p, sweep, True)
    with ss.engine(p, fused) as y:
        ss.setup(y, p)
        sw.whole(y, p, name, kind, five=False)
        want = sw.explicit(y, p, name, kind, sweep, up, lam, new_rows=new_rows, every_step=more, pay=payB, q=p2)
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        sw.whole(e, p, name, kind)
        snap = sw.buffers(e)
        e.update_keypoints_rows(up, [new_rows[0], new_rows[4]])
        bad = Outputs(e)
        pl = sw.pinned_lam(e, lam)
        with pytest.raises(Exception) as err:                    # the sweep list holds pending trajectory 0, the upload list does not
            sw.call5(e, bad, 3, pl, p["eps"], sweep=sweep, upload=[4], **sw.listed_inputs(e, p2, name, kind, [4], every_step=more, pay=payB))
        assert err.value.code == _lib.ERR_STATE and "trajectory 0" in str(err.value), str(err.value)
        with pytest.raises(Exception) as err:                    # no payload at all: nothing may read the pending ranges
            sw.call5(e, bad, 3, pl, p["eps"], sweep=sweep)
        assert err.value.code == _lib.ERR_STATE and "first: 0" in str(err.value), str(err.value)
        e.sync()
        bad.untouched()
        out, after = sw.streamed(e, p, name, kind, sweep, up, lam, 3, gain=sweep,
                                 inputs=sw.listed_inputs(e, p2, name, kind, up, every_step=more, pay=payB))
        sw.check_compact(out, sweep, sweep, want, what=kind)
        sw.check_buffers(after, snap, want, sweep, what=kind)
        again, after2 = sw.streamed(e, p, name, kind, sweep, [], lam, 3, gain=sweep)       # nothing is pending any more
        sw.check_compact(again, sweep, sweep, want, what=(kind, "again"))


# ---- 7. a raw payload on a fused context ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda7", "ragged5"])
def test_raw_payload_on_a_fused_context(name, monkeypatch):
    """x+- records for a list: the chunks difference their own entry ranges, the column store is valid afterwards, and a following
    kpilqr_iterate_partial reads it: the bits of a context that went the explicit route all the way"""
    sw.set_form(monkeypatch, "one_wave")
    p, kind, fused = problem(name), "fd_kp", True
    B = p["batch"]
    sweep, then = SWEEP_LISTS[B][3], SWEEP_LISTS[B][2]
    lam, lam2 = sw.lam_for(p, sweep, True), sw.lam_for(p, then, True) * 1.3
    with ss.engine(p, fused) as y:
        ss.setup(y, p)
        sw.whole(y, p, name, kind, five=False)
        want = sw.explicit(y, p, name, kind, sweep, sweep, lam)
        want2 = sw.explicit(y, p, name, kind, then, [], lam2)
        want_launch = sw.launches(y)
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        sw.whole(e, p, name, kind, 2)
        snap = sw.buffers(e)
        out, after = sw.streamed(e, p, name, kind, sweep, sweep, lam, 2, gain=sweep)
        sw.check_compact(out, sweep, sweep, want, what="raw")
        sw.check_buffers(after, snap, want, sweep, what="raw")
        e.iterate_partial(then, lam2, 100, None)
        got = sw.buffers(e)
        assert sw.launches(e) == want_launch and sw.launches(e)[2] == "in_sweep:subset" and ":kpc:" in sw.launches(e)[0]
        for key in sw.BUFS:
            assert same(got[key], want2[key]), key


# ---- 8. lambda retry ---------------------------------------------------------------------------------------------------------------------
def test_lambda_retry(monkeypatch):
    """The failing problem and schedule of tests/test_gpu_streamed_subset.py::test_combined_with_lambda_retry (on the CPU oracle data
    set A takes 3, 2, 1, 6, 3, 1, 2 sweeps from these lambdas).  First one whole pass under a schedule of ONE attempt: whoever needs more
    keeps a failing status.  Then the real schedule and trajectories {0, 2, 3} listed."""
    sw.set_form(monkeypatch, "one_wave")
    name, fused, kind = "panda7", True, "cols"
    p = dict(problem(name))
    p["w_run"] = -(np.abs(p["w_run"]) + 1.0) * 20.0
    retry = dict(factor=10.0, max_lambda=10.0, max_attempts=6)
    lam0 = np.array([0.1, 1.0, 10.0, 1e-4, 0.1, 10.0, 1.0])
    sweep = [0, 2, 3]
    rest = [1, 4, 5, 6]
    state = {}
    for who in ("y", "e"):
        with ss.engine(p, fused) as e:
            ss.setup(e, p)
            e.set_lambda_retry(factor=10.0, max_lambda=10.0, max_attempts=1)
            sw.whole(e, p, name, kind, lam=lam0, pd_stride=10, five=who == "e")
            snap = sw.buffers(e)
            lam_snap, att_snap = e.lambda_retry()
            e.set_lambda_retry(**retry)
            if who == "y":
                after = sw.explicit(e, p, name, kind, sweep, [], lam0[sweep], pd_stride=10)
            else:
                out, after = sw.streamed(e, p, name, kind, sweep, [], lam0[sweep], 3, gain=sweep, pd_stride=10)
            state[who] = dict(snap=snap, after=after, retry=e.lambda_retry(), lam_snap=lam_snap, att_snap=att_snap)
    y, e = state["y"], state["e"]
    att = y["retry"][1]
    print("explicit route: attempts", att, "status", y["after"]["status"], "status before", y["snap"]["status"])
    assert att[0] > 1 and y["after"]["status"][0] == 0          # fails its first sweep, settles later
    assert att[2] == 1 and y["after"]["status"][2] == 0         # settles at once
    assert y["snap"]["status"][1] != 0                           # an unlisted trajectory whose earlier sweep failed
    assert same(e["after"]["status"], y["after"]["status"])
    assert same(e["retry"][0][sweep], y["retry"][0][sweep]) and same(e["retry"][1][sweep], y["retry"][1][sweep])
    assert same(e["retry"][0][rest], e["lam_snap"][rest]) and same(e["retry"][1][rest], e["att_snap"][rest])
    sw.check_compact(out, sweep, sweep, y["after"], what="retry")
    sw.check_buffers(e["after"], e["snap"], y["after"], sweep, what="retry")


# ---- 9. K32 and a gain list that differs from the sweep list ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("panda7", True), ("panda5rec", False)])
def test_k32_and_a_gain_list_of_its_own(name, fused, monkeypatch):
    sw.set_form(monkeypatch, "one_wave")
    p, kind = problem(name), "cols32"
    B = p["batch"]
    sweep, gain = SWEEP_LISTS[B][2], [3, B - 1]                  # nobody of the gain list is swept
    assert not set(sweep) & set(gain)
    lam = sw.lam_for(p, sweep, True)
    with ss.engine(p, fused) as y:
        ss.setup(y, p)
        sw.whole(y, p, name, kind, five=False)
        want = sw.explicit(y, p, name, kind, sweep, sweep[:1], lam)
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        for f32, g in ((True, gain), (False, gain), (True, None), (True, sweep)):
            sw.whole(e, p, name, kind)
            snap = sw.buffers(e)
            out, after = sw.streamed(e, p, name, kind, sweep, sweep[:1], lam, 3, gain=g, f32=f32)
            sw.check_compact(out, sweep, g, want, f32=f32, what=(f32, g))
            sw.check_buffers(after, snap, want, sweep, what=(f32, g))
            if g == gain:                                        # the gains of an unswept trajectory: the resident bits
                assert same(after["K"][gain], snap["K"][gain])


# ---- 10. rejections change nothing -----------------------------------------------------------------------------------------------------
def raw_io5(e, out, lam, eps, sweep, rows=None, up=None, kind=None, pay=None, entries=0):
    io5 = _lib.StreamIO5()
    io5.struct_size = C.sizeof(_lib.StreamIO5)
    io4 = ss.raw_io4(e, out, lam, eps, rows, up, kind, pay, entries)
    C.memmove(C.byref(io5.io4), C.byref(io4), C.sizeof(_lib.StreamIO4))
    if sweep is not None:
        io5.sweep_count = len(sweep)
        io5.sweep_traj = sweep.ctypes.data
    return io5


def test_rejected_calls_change_nothing(monkeypatch):
    sw.set_form(monkeypatch, "one_wave")
    name, fused, kind = "panda7", True, "cols"
    p = problem(name)
    B = p["batch"]
    sweep, up = np.array([1, 3, 5], np.int32), np.array([1, 5], np.int32)
    good = [1, 3, 5]
    lam_good = sw.lam_for(p, good, True)
    with ss.engine(p, fused) as y:                                # a context that never sees a refused call
        ss.setup(y, p)
        sw.whole(y, p, name, kind)
        _, want = sw.streamed(y, p, name, kind, good, [], lam_good, 3, gain=good)
    with ss.engine(p, fused) as e:
        lam = e.pinned(B); lam[:] = p["lam"]
        first = Outputs(e)
        io5 = raw_io5(e, first, lam, p["eps"], sweep)
        assert e._L.kpilqr_iterate_streamed5(e._h, C.byref(io5), 100, 3) == _lib.ERR_STATE      # before any key-points exist
        first.untouched()
        ss.setup(e, p)
        sw.whole(e, p, name, kind)
        snap = sw.buffers(e)
        idx = ss.entry_index(p, up)
        E = len(idx)
        pay = ss.pin_payload(e, kind, ss.take(ss.payload_of(name, p, kind, "B"), idx))
        rows = ss.pin_rows(e, ss.rows_of(p, "B"), up)
        whole_fd = e.fd_slab(p["job_b"], p["job_t"], p["job_col"], p["job_mode"], p["xplus"], p["xminus"], p["job_nom"], p["xnom"])
        lists = dict(decreasing=np.array([5, 3, 1], np.int32), repeated=np.array([1, 1, 5], np.int32), beyond=np.array([1, 5, B], np.int32),
                     negative=np.array([-1, 1, 5], np.int32))
        missing = np.array([1, 3], np.int32)                      # upload list [1, 5]: trajectory 5 is not swept

        def fd_slab(io5):
            io = io5.io4.io3.io2.io
            io.kp_columns = None; io.entries = 0
            io5.io4.upload_traj = None; io5.io4.upload_count = 0
            for k in ss.ROWS:
                setattr(io, k, None)
            io.fd_slab = whole_fd["slab"].ctypes.data; io.njobs = whole_fd["njobs"]; io.nnom = whole_fd["nnom"]
            io.traj_job_first = whole_fd["traj_job_first"].ctypes.data; io.traj_nom_first = whole_fd["traj_nom_first"].ctypes.data

        def no_upload_list(io5):
            io5.io4.upload_traj = None; io5.io4.upload_count = 0

        def rows_alone(io5):
            no_upload_list(io5)
            io5.io4.io3.io2.io.kp_columns = None; io5.io4.io3.io2.io.entries = 0

        bad = {
            "outer struct_size + 8": (_lib.ERR_ARG, lambda io5: setattr(io5, "struct_size", C.sizeof(_lib.StreamIO5) + 8), 100),
            "io4 struct_size - 8": (_lib.ERR_ARG, lambda io5: setattr(io5.io4, "struct_size", C.sizeof(_lib.StreamIO4) - 8), 100),
            "io3 struct_size + 8": (_lib.ERR_ARG, lambda io5: setattr(io5.io4.io3, "struct_size", C.sizeof(_lib.StreamIO3) + 8), 100),
            "io2 struct_size + 8": (_lib.ERR_ARG, lambda io5: setattr(io5.io4.io3.io2, "struct_size", C.sizeof(_lib.StreamIO2) + 8), 100),
            "sweep_count < 0": (_lib.ERR_ARG, lambda io5: setattr(io5, "sweep_count", -1), 100),
            "count without a list": (_lib.ERR_ARG, lambda io5: setattr(io5, "sweep_traj", None), 100),
            "pd_check_stride 0": (_lib.ERR_ARG, lambda io5: None, 0),
            "payload and rows without upload_traj": (_lib.ERR_ARG, no_upload_list, 100),
            "rows without upload_traj": (_lib.ERR_ARG, rows_alone, 100),
            "upload entry missing from sweep_traj": (_lib.ERR_ARG, lambda io5: (setattr(io5, "sweep_traj", missing.ctypes.data), setattr(io5, "sweep_count", 2)), 100),
            "fd_slab with a sweep list": (_lib.ERR_ARG, fd_slab, 100),
        }
        for key, arr in lists.items():
            bad["list " + key] = (_lib.ERR_ARG, lambda io5, arr=arr: setattr(io5, "sweep_traj", arr.ctypes.data), 100)
        for what, (code, spoil, stride) in bad.items():
            out = Outputs(e)
            io5 = raw_io5(e, out, lam, p["eps"], sweep, rows, up, kind, pay, E)
            spoil(io5)
            rc = e._L.kpilqr_iterate_streamed5(e._h, C.byref(io5), stride, 3)
            assert rc == code, (what, rc, e._L.kpilqr_strerror(e._h))
            if "missing" in what:
                assert "trajectory 5" in e._L.kpilqr_strerror(e._h).decode()
            e.sync()
            out.untouched()
            now = sw.buffers(e)
            for k in sw.BUFS:
                assert same(now[k], snap[k]), (what, k)
            ok, after = sw.streamed(e, p, name, kind, good, [], lam_good, 3, gain=good)      # the next call: the bits of the untouched context
            sw.check_compact(ok, good, good, want, what=what)
            sw.whole(e, p, name, kind)
        assert e._L.kpilqr_iterate_streamed5(e._h, None, 100, 3) == _lib.ERR_ARG


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_a_rejected_r_x_leaves_the_constant_jacobian_mode(fused, monkeypatch):
    sw.set_form(monkeypatch, "one_wave")
    name = "panda7" if fused else "panda5rec"
    p = problem(name, False)                                     # reaching residuals: one constant r_x, r_u = 0
    cols = ss.columns(name, 1.0, False)[0]
    sweep, up = SWEEP_LISTS[p["batch"]][3], SWEEP_LISTS[p["batch"]][3][:1]
    lam = sw.lam_for(p, sweep, True)
    got = {}
    for refused in (False, True):
        with ss.engine(p, fused) as e:
            ss.setup(e, p)
            e.upload_residual_jacobians_const(p["rx_const"], None)
            pl = ss.lam_of(e, p)
            first = Outputs(e)
            sw.call5(e, first, 3, pl, p["eps"], **ss.pin_rows(e, dict(r=np.array(p["r"]), u_nom=np.array(p["u_nom"]))),
                     **ss.pin_payload(e, "cols", (cols,)))
            e.sync()
            if refused:
                rx = e.pinned((len(up),) + p["r_x"].shape[1:]); rx[...] = 0.5
                out = Outputs(e)
                with pytest.raises(Exception) as err:
                    sw.call5(e, out, 3, sw.pinned_lam(e, lam), p["eps"], sweep=sweep, upload=up, r_x=rx)
                assert err.value.code == _lib.ERR_STATE and "constant residual Jacobians" in str(err.value), str(err.value)
                e.sync()
                out.untouched()
            out = Outputs(e)
            sw.call5(e, out, 3, sw.pinned_lam(e, lam), p["eps"], sweep=sweep, gain=sweep)
            e.sync()
            got[refused] = dict(buf=sw.buffers(e), launch=sw.launches(e), cost=out.rows("cost_pred", len(sweep)).copy())
    assert got[True]["launch"] == got[False]["launch"]
    if fused:
        assert all(":rxc" in s for s in got[True]["launch"][:2]), got[True]["launch"]
    for key in sw.BUFS:
        assert same(got[True]["buf"][key], got[False]["buf"][key]), key
    assert same(got[True]["cost"], got[False]["cost"])


# ---- 11. the other linearisation routes of a context with records, and resident job lists ------------------------------------------------
@pytest.mark.parametrize("kind", ["cols", "fd_kp"])
@pytest.mark.parametrize("name", ["panda5rec", "ragged5"])
def test_three_pass_linearisation(name, kind, monkeypatch):
    """KPILQR_FD_INTERP=0 (diagnostic): the listed linearisation is columns -> the listed key-point steps -> k_interpolate, and a raw
    payload is differenced into the chunk's range of the column store first"""
    monkeypatch.setenv("KPILQR_FD_INTERP", "0")                  # (read when a context is created)
    p, fused = problem(name), False
    B = p["batch"]
    with ss.engine(p, fused) as e, ss.engine(p, fused) as y:
        ss.setup(e, p); ss.setup(y, p)
        for sweep, upload in ((SWEEP_LISTS[B][3], SWEEP_LISTS[B][3]), (SWEEP_LISTS[B][2], [])):
            lam = sw.lam_for(p, sweep, True)
            sw.whole(y, p, name, kind, five=False)
            want = sw.explicit(y, p, name, kind, sweep, upload, lam)
            want_launch = sw.launches(y)
            for nchunks in (2, 3):
                sw.whole(e, p, name, kind, nchunks)
                snap = sw.buffers(e)
                out, after = sw.streamed(e, p, name, kind, sweep, upload, lam, nchunks, gain=sweep)
                sw.check_compact(out, sweep, sweep, want, what=(sweep, nchunks))
                sw.check_buffers(after, snap, want, sweep, what=(sweep, nchunks))
                assert sw.launches(e) == want_launch and want_launch[2] == "fd_difference+interpolate:subset", sw.launches(e)


@pytest.mark.parametrize("name,fused", [("panda7", True), ("panda5rec", False)])
def test_resident_job_lists(name, fused, monkeypatch):
    """A job-list payload resident from the explicit calls: a sweep list alone (no upload) sweeps the listed trajectories on it"""
    sw.set_form(monkeypatch, "one_wave")
    p = problem(name)
    B = p["batch"]
    sweep = SWEEP_LISTS[B][3]
    lam = sw.lam_for(p, sweep, True)
    bufs = {}
    for who in ("y", "e"):
        with ss.engine(p, fused) as e:
            ss.setup(e, p)
            e.upload_fd(p["job_b"], p["job_t"], p["job_col"], p["job_mode"], p["xplus"], p["xminus"], job_nom=p["job_nom"], xnom=p["xnom"],
                        eps=p["eps"])
            e.upload_residuals(p["r"], p["r_x"], p["r_u"])
            e.upload_nominal(p["u_nom"])
            e.iterate(p["lam"], 100, None)
            snap = sw.buffers(e)
            if who == "y":
                e.iterate_partial(sweep, lam, 100, None)
                after = sw.buffers(e)
            else:
                out, after = sw.streamed(e, p, name, "cols", sweep, [], lam, 3, gain=sweep)
            bufs[who] = dict(snap=snap, after=after, launch=sw.launches(e))
    assert np.all(bufs["y"]["after"]["status"][sweep] == 0) and bufs["e"]["launch"] == bufs["y"]["launch"], bufs["e"]["launch"]
    sw.check_compact(out, sweep, sweep, bufs["y"]["after"], what="jobs")
    sw.check_buffers(bufs["e"]["after"], bufs["e"]["snap"], bufs["y"]["after"], sweep, what="jobs")
    assert not same(bufs["e"]["after"]["K"][sweep], bufs["e"]["snap"]["K"][sweep])
