"""GPU tests of kpilqr_iterate_streamed4 (csrc/rows_in.hip: k_rows_in; csrc/columns_f32.hip with a list): the chunk pipeline uploading
the inputs of a LISTED subset of the batch -- per chunk and array one upload of the compact slice into a staging region, one launch
that moves the rows to their trajectories' places.

The yardstick is never the code under test: a fresh context (tests/_streamed_subset.py: Yardstick) that runs kpilqr_iterate_streamed3,
three chunks, on whole-batch arrays holding data set A with the listed rows / entries replaced by data set B's.  Those are the same
kernels on the same device bytes, so K, k, cost_pred, delta_J and status must be its bits, and the kpilqr_last_launch strings its
strings.  Where the payload is a column kind, K and k of every trajectory whose oracle status is 0 are also held to the C oracle at
the suite's 1e-9.

Shapes, contexts and sentinel-guarded outputs are those of tests/test_gpu_streamed_columns_f32.py (panda7, acrobot3, panda5rec,
pushing3, ragged5 fused and with records).  With three chunks the batches are cut [0,2) [2,4) [4,7) | [0,1) [1,3) [3,5) | one each."""
import ctypes as C

import numpy as np
import pytest

import _streamed_subset as ss
from _streamed_subset import CONTEXTS, IDS, KINDS, Outputs, Yardstick, check, problem, same
from test_gpu_streamed_columns_f32 import ragged_rows
from trajoptkp_amd import _lib, synth

pytestmark = pytest.mark.gpu

# first | last | a pair straddling a chunk boundary (three chunks) | a scattered pair | all | empty
UPLOAD_LISTS = {7: [[0], [6], [1, 2], [1, 5], list(range(7)), []], 5: [[0], [4], [0, 1], [0, 3], list(range(5)), []],
                3: [[0], [2], [0, 1], [0, 2], [0, 1, 2], []]}
BUFFERS = (("r", _lib.BUF_RESIDUALS), ("r_x", _lib.BUF_R_X), ("u_nom", _lib.BUF_U_NOM))


def start(e, p, name, kind, nchunks=3):
    """data set A through a whole call (upload_traj = None); returns lam"""
    lam = ss.lam_of(e, p)
    out = Outputs(e)
    ss.call(e, out, nchunks, lam, p["eps"], **ss.pin_rows(e, ss.rows_of(p, "A")),
            **ss.pin_payload(e, kind, ss.payload_of(name, p, kind, "A")))
    return lam


def listed_inputs(e, p, name, kind, pay_list, row_list, which="B", every_step=(4,), keys=ss.ROWS):
    """the compact pinned inputs of a listed call: B's payload entries of pay_list, B's rows of row_list (one list or None each)"""
    kw = {}
    if pay_list is not None:
        pay = ss.payload_of(name, p, kind, which, every_step)
        kw.update(ss.pin_payload(e, kind, ss.take(pay, ss.entry_index(p, pay_list))))
    if row_list is not None:
        rows = ss.rows_of(p, which)
        kw.update(ss.pin_rows(e, dict((k, rows[k]) for k in keys), row_list))
    return kw


# ---- 1. + 2. a subset equals the whole call on the mixed arrays, and nothing else is written -----------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,fused", CONTEXTS, ids=IDS)
def test_subset_equals_whole(name, fused, kind):
    p = problem(name)
    B = p["batch"]
    A_rows, B_rows = ss.rows_of(p, "A"), ss.rows_of(p, "B")
    held = 0
    with Yardstick(name, fused, kind) as yard, ss.engine(p, fused) as e:
        ss.setup(e, p)
        # (payload list, row list, chunk counts): all together at every chunk count; the payload alone and r / u_nom alone at three
        cases = [(tr, tr, ss.chunk_counts(B)) for tr in UPLOAD_LISTS[B]]
        cases += [(tr, None, [3]) for tr in UPLOAD_LISTS[B][2:4]] + [(None, tr, [3]) for tr in UPLOAD_LISTS[B][2:4]]
        for pay_list, row_list, counts in cases:
            traj = pay_list if pay_list is not None else row_list
            ref = yard.mixed(pay_list, row_list)
            keys = ss.ROWS if pay_list is not None else ("r", "u_nom")
            if pay_list is None:                                  # r and u_nom alone: r_x and r_u stay A's for everybody, and no payload
                rows = dict(A_rows); rows["r"] = ref["rows"]["r"]; rows["u_nom"] = ref["rows"]["u_nom"]
                yard.run(A_rows, ref["pay"])                      # comes: the whole call brings none either, behind one that brought A's
                ref = dict(yard.run(rows, None), rows=rows, pay=ref["pay"])
            for nchunks in counts:
                lam = start(e, p, name, kind, nchunks)
                out = Outputs(e)
                ss.call(e, out, nchunks, lam, p["eps"], upload_traj=traj, **listed_inputs(e, p, name, kind, pay_list, row_list, keys=keys))
                e.sync()
                what = (pay_list, row_list, nchunks)
                check(out, ref, what=what)
                assert ss.launches(e) == ref["launch"], (what, ss.launches(e), ref["launch"])
                # nothing else written: the device buffers hold B's bits for the listed rows and A's for everybody else
                for key, which in BUFFERS:
                    got = e._d2h(which, ref["rows"][key].shape, np.float64)
                    assert same(got, ref["rows"][key]), (what, key)
                    kept = [b for b in range(B) if row_list is None or b not in row_list or key not in keys]
                    assert same(got[kept], A_rows[key][kept]), (what, key, "a kept trajectory was written")
                    if row_list and key in keys:
                        assert same(got[row_list], B_rows[key][row_list]) and not same(got[row_list], A_rows[key][row_list])
            cols = ss.decoded_columns(name, p, kind, ref["pay"]) if pay_list in ([1, 2], [0, 1]) and row_list else None
            if cols is not None:
                held += ss.hold_to_oracle(p, ref["rows"], cols, ss.taken(out), f"{name} fused={fused} {kind} {traj}")
        # (the mixtures are other problems than A and than B)
        assert not same(yard.mixed(UPLOAD_LISTS[B][0], UPLOAD_LISTS[B][0])["K"], yard.mixed([], [])["K"])
    assert kind == "fd_kp" or held > 0


# ---- 3. changed key-point lists ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_changed_lists(fused, kind):
    """ragged5: trajectories {0, 4} get new lists (0: a key-point at every step, 549 -> 725 entries; 4: its own list again), then the payload of
    {0, 4}, or of the superset {0, 2, 4}, completes the pending ranges: the bits of a fresh context on the merged lists"""
    name, more = "ragged5", (0, 4)
    p, p2 = problem(name), problem(name, True, more)
    assert ss.first_entries(p)[-1] == 549 and ss.first_entries(p2)[-1] == 725
    new_rows = ragged_rows(more)
    f1, f2 = ss.first_entries(p), ss.first_entries(p2)
    payA = ss.payload_of(name, p, kind, "A")
    payB = ss.payload_of(name, p2, kind, "B", more)
    with Yardstick(name, fused, kind, p=p) as yard:              # a fresh context of the same problem ...
        yard.e.set_keypoints_rows(p2["kp_rows"])                 # ... on the merged lists
        for traj in ([0, 4], [0, 2, 4]):
            # the merged payload: what was resident for the kept trajectories (their entries move, their bytes stay), B's for the listed
            pay = tuple(y.copy() for y in payB)
            for b in range(p["batch"]):
                if b not in traj:
                    assert f1[b + 1] - f1[b] == f2[b + 1] - f2[b]
                    for x, y in zip(pay, payA):
                        x[f2[b]:f2[b + 1]] = y[f1[b]:f1[b + 1]]
            ref = yard.run(ss.rows_of(p, "A"), pay)
            with ss.engine(p, fused) as e:
                ss.setup(e, p)
                lam = start(e, p, name, kind)
                e.update_keypoints_rows([0, 4], [new_rows[0], new_rows[4]])
                if traj == [0, 4]:                               # a list that misses a pending trajectory
                    bad = Outputs(e)
                    with pytest.raises(Exception) as err:
                        ss.call(e, bad, 3, lam, p["eps"], upload_traj=[4], **ss.pin_payload(e, kind, ss.take(payB, ss.entry_index(p2, [4]))))
                    assert err.value.code == _lib.ERR_STATE and "trajectory 0" in str(err.value), str(err.value)
                    e.sync()
                    bad.untouched()
                    with pytest.raises(Exception) as err:        # still pending: nothing may read the payload
                        ss.call(e, bad, 3, lam, p["eps"], upload_traj=[])
                    assert err.value.code == _lib.ERR_STATE
                out = Outputs(e)
                ss.call(e, out, 3, lam, p["eps"], upload_traj=traj, **ss.pin_payload(e, kind, ss.take(payB, ss.entry_index(p2, traj))))
                e.sync()
                check(out, ref, what=(kind, traj))
                assert ss.launches(e) == ref["launch"]
                again = Outputs(e)                               # nothing is pending any more: an iteration without a payload
                ss.call(e, again, 3, lam, p["eps"], upload_traj=[])
                e.sync()
                check(again, ref, what=(kind, traj, "again"))


# ---- 4. two calls in flight with different lists and different data, then the staging grows -------------------------------------------
@pytest.mark.parametrize("kind", ["cols", "fd_kp", "cols32"])
@pytest.mark.parametrize("name,fused", [("panda7", True), ("panda5rec", False), ("ragged5", True)])
def test_calls_in_flight_with_different_lists(name, fused, kind):
    """Three calls and ONE wait.  The first two list different trajectories and bring different data (payload, r, u_nom); the third lists
    everybody and brings r_x and r_u as well, whose staging regions do not exist yet: the library has to reserve them behind the two
    calls in flight.  Then the ring of lists goes round."""
    p = problem(name)
    B = p["batch"]
    l1, l2, l3 = UPLOAD_LISTS[B][2], [B - 1], list(range(B))
    few = ("r", "u_nom")
    rowsA, rowsB = ss.rows_of(p, "A"), ss.rows_of(p, "B")
    rowsC = dict((k, v * 1.02 + 0.001) for k, v in rowsB.items())
    payA, payB = ss.payload_of(name, p, kind, "A"), ss.payload_of(name, p, kind, "B")
    if kind == "fd_kp":
        payC = (payB[1] + 0.5 * (payB[0] - payB[1]), payB[1], payB[2])
    else:
        payC = (ss.columns(name, 0.5)[0 if kind == "cols" else 1].copy(),)
    idx2 = ss.entry_index(p, l2)
    with Yardstick(name, fused, kind) as yard:
        rows1 = dict((k, v.copy()) for k, v in rowsA.items())
        for k in few:
            rows1[k][l1] = rowsB[k][l1]
        pay1 = ss.mix(payA, payB, ss.entry_index(p, l1))
        ref1 = yard.run(rows1, pay1)
        rows2 = dict((k, v.copy()) for k, v in rows1.items())
        for k in few:
            rows2[k][l2] = rowsC[k][l2]
        pay2 = ss.mix(pay1, payC, idx2)
        ref2 = yard.run(rows2, pay2)
        ref3 = yard.mixed(l3, l3)                                           # everybody listed, every array: B throughout
    assert not same(ref1["K"], ref2["K"]) and not same(ref2["K"], ref3["K"])
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        in1 = listed_inputs(e, p, name, kind, l1, l1, keys=few)
        in2 = dict(ss.pin_payload(e, kind, ss.take(payC, idx2)), **ss.pin_rows(e, dict((k, rowsC[k]) for k in few), l2))
        in3 = listed_inputs(e, p, name, kind, l3, l3)
        outs = [Outputs(e) for _ in range(3)]
        lam = start(e, p, name, kind)
        ss.call(e, outs[0], 3, lam, p["eps"], upload_traj=l1, **in1)
        ss.call(e, outs[1], 3, lam, p["eps"], upload_traj=l2, **in2)      # no wait: staging is addressed by the chunk, the list has a ring
        ss.call(e, outs[2], 3, lam, p["eps"], upload_traj=l3, **in3)      # the staging of r_x and r_u is reserved behind the calls in flight
        e.sync()
        check(outs[0], ref1, what="first")
        check(outs[1], ref2, what="second")
        check(outs[2], ref3, what="third")
        for i in range(6):                                                # the ring of lists goes round: alternate lists, one wait
            ss.call(e, outs[i % 2], 3, lam, p["eps"], upload_traj=[l1, l3][i % 2], **[in1, in3][i % 2])
        e.sync()
        # (B's rows and entries for l1 on top of everybody's B change nothing)
        check(outs[0], ref3, what="ring, l1")
        check(outs[1], ref3, what="ring, l3")


# ---- 5. with K32, the gains of a list, and the lambda retry schedule -----------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("panda7", True), ("panda5rec", False), ("pushing3", False), ("ragged5", True)])
def test_combined_with_k32_and_gain_lists(name, fused):
    p, kind = problem(name), "cols32"
    B = p["batch"]
    up = UPLOAD_LISTS[B][3]
    with Yardstick(name, fused, kind) as yard:
        ref = yard.mixed(up, up)
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        inp = listed_inputs(e, p, name, kind, up, up)
        for i, gain in enumerate([None] + ss.LISTS[B]):
            f32 = not i % 2
            lam = start(e, p, name, kind)
            out = Outputs(e)
            ss.call(e, out, 3, lam, p["eps"], upload_traj=up, gain=gain, f32=f32, **inp)
            e.sync()
            check(out, ref, traj=gain, f32=f32, what=(gain, f32))


def test_combined_with_lambda_retry():
    """panda7 under a retry schedule with the failing inputs of the lambda retry tests (negative running weights, per-trajectory start
    lambdas, a PD check every 10 steps; on the CPU oracle the first data set then takes 3, 2, 1, 6, 3, 1, 2 sweeps): the bits, the
    lambdas used and the attempt counts of the yardstick under the same schedule"""
    name, fused, kind = "panda7", True, "cols"
    p = dict(problem(name))
    p["w_run"] = -(np.abs(p["w_run"]) + 1.0) * 20.0
    up = [1, 5]
    retry = dict(factor=10.0, max_lambda=10.0, max_attempts=6)
    lam0 = np.array([0.1, 1.0, 10.0, 1e-4, 0.1, 10.0, 1.0])
    with Yardstick(name, fused, kind, p=p, retry=retry, pd_stride=10) as yard:
        yard.lam[:] = lam0
        ref = yard.mixed(up, up)
        want = yard.e.lambda_retry()
    print("attempts under the schedule:", want[1], "status:", ref["status"])
    assert np.max(want[1]) > 2 and np.min(want[1]) == 1          # (the yardstick: some trajectories settle at once, some after retries)
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        e.set_lambda_retry(**retry)
        lam = start(e, p, name, kind)
        e.sync()
        lam[:] = lam0
        out = Outputs(e)
        ss.call(e, out, 3, lam, p["eps"], upload_traj=up, pd_stride=10, **listed_inputs(e, p, name, kind, up, up))
        e.sync()
        check(out, ref, what="retry")
        got = e.lambda_retry()
        assert same(np.asarray(got[0]), np.asarray(want[0])) and np.array_equal(got[1], want[1])


# ---- 6. the uploads follow KPILQR_PIPE_COPY -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe_copy", ["0", "1", "3"])
def test_upload_follows_the_pipe_copy_switch(pipe_copy, monkeypatch):
    """panda7, two chunks [0,3) [3,7), list [1, 3, 6]: the second chunk's slice starts one u_nom row (119 doubles) into the caller's
    compact array -- 8 mod 16 bytes -- and lands three rows into the staging region -- 8 mod 16 bytes as well"""
    name, fused = "panda7", True
    p = problem(name)
    assert (p["T"] * p["m"]) % 2 == 1 and (p["T"] * p["m"] * 8) % 16 == 8
    up = [1, 3, 6]
    for kind in KINDS:
        with Yardstick(name, fused, kind) as yard:
            ref = yard.mixed(up, up)
        monkeypatch.setenv("KPILQR_PIPE_COPY", pipe_copy)       # read when the context is created
        with ss.engine(p, fused) as e:
            ss.setup(e, p)
            inp = listed_inputs(e, p, name, kind, up, up)
            for nchunks in (2, 3):
                lam = start(e, p, name, kind, nchunks)
                out = Outputs(e)
                ss.call(e, out, nchunks, lam, p["eps"], upload_traj=up, **inp)
                e.sync()
                check(out, ref, what=(pipe_copy, kind, nchunks))
        monkeypatch.delenv("KPILQR_PIPE_COPY")


# ---- 7. upload_traj = NULL is kpilqr_iterate_streamed3 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("panda7", True), ("panda5rec", False)])
def test_null_list_is_streamed3(name, fused):
    p = problem(name)
    got = {}
    for four in (False, True):
        with ss.engine(p, fused) as e:
            ss.setup(e, p)
            lam = ss.lam_of(e, p)
            for i, (kind, gain, f32) in enumerate((("cols32", None, False), ("fd_kp", [1, 2], True), ("cols", None, False))):
                out = Outputs(e)
                ss.call(e, out, 3, lam, p["eps"], gain=gain, f32=f32, four=four, **ss.pin_rows(e, ss.rows_of(p, "A")),
                        **ss.pin_payload(e, kind, ss.payload_of(name, p, kind, "A")))
                e.sync()
                count = None if gain is None else len(gain)
                res = dict((n, out.rows(n).copy()) for n in ("cost_pred", "delta_J", "status"))
                res["K"] = out.rows("K32" if f32 else "K", count).copy()
                res["k"] = out.rows("k", count).copy()
                res["launch"] = ss.launches(e)
                got[four, i] = res
    for i in range(3):
        old, new = got[False, i], got[True, i]
        assert old["launch"] == new["launch"]
        for key in ss.OUT:
            assert same(new[key], old[key]), (i, key)
    assert np.all(got[False, 0]["status"] == 0) and np.any(got[False, 0]["K"] != 0)


# ---- 8. rejections leave everything alone ----------------------------------------------------------------------------------------------
def test_rejected_calls_change_nothing():
    name, fused, kind = "panda7", True, "cols"
    p = problem(name)
    B = p["batch"]
    up = np.array([1, 5], np.int32)
    with Yardstick(name, fused, kind) as yard:
        refA = yard.mixed(None, None)
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        lam = start(e, p, name, kind)
        e.sync()
        payB = ss.payload_of(name, p, kind, "B")
        idx = ss.entry_index(p, up)
        E = len(idx)
        pay = ss.pin_payload(e, kind, ss.take(payB, idx))
        pay32 = ss.pin_payload(e, "cols32", ss.take(ss.payload_of(name, p, "cols32", "B"), idx))
        slab = ss.pin_payload(e, "fd_kp", ss.take(ss.payload_of(name, p, "fd_kp", "B"), idx))
        rows = ss.pin_rows(e, ss.rows_of(p, "B"), up)
        whole_fd = e.fd_slab(p["job_b"], p["job_t"], p["job_col"], p["job_mode"], p["xplus"], p["xminus"], p["job_nom"], p["xnom"])
        lists = dict(decreasing=np.array([5, 1], np.int32), repeated=np.array([1, 1], np.int32), beyond=np.array([1, B], np.int32),
                     negative=np.array([-1, 5], np.int32))

        def fd_slab(io4):
            io = io4.io3.io2.io
            io.kp_columns = None; io.entries = 0
            io.fd_slab = whole_fd["slab"].ctypes.data; io.njobs = whole_fd["njobs"]; io.nnom = whole_fd["nnom"]
            io.traj_job_first = whole_fd["traj_job_first"].ctypes.data; io.traj_nom_first = whole_fd["traj_nom_first"].ctypes.data

        def other_kind(io4):                                    # the resident payload is the column kind: records cannot join it
            io4.io3.io2.io.kp_columns = None
            io4.io3.io2.io.fd_kp_slab = slab["fd_kp"]["slab"].ctypes.data

        bad = {
            "outer struct_size + 8": (_lib.ERR_ARG, lambda io4: setattr(io4, "struct_size", C.sizeof(_lib.StreamIO4) + 8)),
            "io3 struct_size - 8": (_lib.ERR_ARG, lambda io4: setattr(io4.io3, "struct_size", C.sizeof(_lib.StreamIO3) - 8)),
            "io2 struct_size + 8": (_lib.ERR_ARG, lambda io4: setattr(io4.io3.io2, "struct_size", C.sizeof(_lib.StreamIO2) + 8)),
            "upload_count < 0": (_lib.ERR_ARG, lambda io4: setattr(io4, "upload_count", -1)),
            "count without a list": (_lib.ERR_ARG, lambda io4: setattr(io4, "upload_traj", None)),
            "entries + 1": (_lib.ERR_ARG, lambda io4: setattr(io4.io3.io2.io, "entries", E + 1)),
            "entries - 1": (_lib.ERR_ARG, lambda io4: setattr(io4.io3.io2.io, "entries", E - 1)),
            "entries of the whole batch": (_lib.ERR_ARG, lambda io4: setattr(io4.io3.io2.io, "entries", int(ss.first_entries(p)[-1]))),
            "two payloads": (_lib.ERR_ARG, lambda io4: setattr(io4.io3, "kp_columns32", pay32["kp_cols32"].ctypes.data)),
            "fd_slab with a list": (_lib.ERR_ARG, fd_slab),
            "payload of the other kind": (_lib.ERR_STATE, other_kind),
        }
        for key, arr in lists.items():
            bad["list " + key] = (_lib.ERR_ARG, lambda io4, arr=arr: setattr(io4, "upload_traj", arr.ctypes.data))
        for what, (code, spoil) in bad.items():
            out = Outputs(e)
            io4 = ss.raw_io4(e, out, lam, p["eps"], rows, up, kind, pay, E)
            spoil(io4)
            rc = e._L.kpilqr_iterate_streamed4(e._h, C.byref(io4), 100, 3)
            assert rc == code, (what, rc)
            e.sync()
            out.untouched()
            good = Outputs(e)                                    # the next iteration: still data set A for everybody
            ss.call(e, good, 3, lam, p["eps"], upload_traj=[])
            e.sync()
            check(good, refA, what=what)
        assert e._L.kpilqr_iterate_streamed4(e._h, None, 100, 3) == _lib.ERR_ARG


def test_payload_with_a_list_needs_a_resident_payload():
    """no payload yet, and a job-list payload: neither is a complete resident payload of a by-entry kind"""
    name, fused = "panda7", True
    p = problem(name)
    up = [1, 5]
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        lam = ss.lam_of(e, p)
        for kind in KINDS:
            out = Outputs(e)
            with pytest.raises(Exception) as err:
                ss.call(e, out, 3, lam, p["eps"], upload_traj=up, **listed_inputs(e, p, name, kind, up, None))
            assert err.value.code == _lib.ERR_STATE, kind
        e.upload_fd_kp(e.fd_kp_slab(*synth.kp_ordered_payload(p), pinned=False), p["eps"])      # records resident: columns cannot join them
        for kind in ("cols", "cols32"):
            with pytest.raises(Exception) as err:
                ss.call(e, out, 3, lam, p["eps"], upload_traj=up, **listed_inputs(e, p, name, kind, up, None))
            assert err.value.code == _lib.ERR_STATE, kind
        e.sync()
        out.untouched()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "records"])
def test_residual_jacobians_of_a_subset_are_refused_where_the_partial_upload_is(fused):
    """r_x with a list in the constant-Jacobian mode and before a whole r_x, r_u with a list before a whole r_u: KPILQR_ERR_STATE, the
    constant mode survives (fused: the ':rxc' token), and the next iteration gives the bits it gave before"""
    name = "panda7" if fused else "panda5rec"
    p = problem(name, False)                                     # reaching residuals: one constant r_x, r_u = 0
    cols = ss.columns(name, 1.0, False)[0]
    up = [1, 3]
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        lam = ss.lam_of(e, p)
        whole = ss.pin_rows(e, dict(r=np.array(p["r"]), u_nom=np.array(p["u_nom"])))
        rx = e.pinned((len(up),) + p["r_x"].shape[1:]); rx[...] = 0.5
        ru = e.pinned((len(up),) + p["r_u"].shape[1:]); ru[...] = 0.25
        # before any r_x: the buffer's other rows mean nothing yet
        out = Outputs(e)
        with pytest.raises(Exception) as err:
            ss.call(e, out, 3, lam, p["eps"], upload_traj=up, r_x=rx)
        assert err.value.code == _lib.ERR_STATE and "before a whole r_x" in str(err.value)
        e.upload_residual_jacobians_const(p["rx_const"], None)
        want = Outputs(e)
        ss.call(e, want, 3, lam, p["eps"], **whole, **ss.pin_payload(e, "cols", (cols,)))
        e.sync()
        ref = ss.taken(want)
        launches = ss.launches(e)
        if fused:
            assert all(":rxc" in s for s in launches[:2]), launches
        for what, kw, words in (("r_x", dict(r_x=rx), "constant residual Jacobians"), ("r_u", dict(r_u=ru), "without control residuals"),
                                ("r_x, nobody listed", dict(r_x=rx), "constant residual Jacobians")):
            out = Outputs(e)
            with pytest.raises(Exception) as err:
                ss.call(e, out, 3, lam, p["eps"], upload_traj=[] if "nobody" in what else up, **kw)
            assert err.value.code == _lib.ERR_STATE and words in str(err.value), (what, str(err.value))
            e.sync()
            out.untouched()
            got = Outputs(e)
            ss.call(e, got, 3, lam, p["eps"], upload_traj=[])
            e.sync()
            check(got, ref, what=what)
            assert ss.launches(e)[:2] == launches[:2], what


def test_records_then_columns_with_lists_in_flight():
    """A listed call with x+- records, a whole call with FP64 columns, a listed call with columns, no wait in between: the payload
    staging region is cut by another record size, which the library orders behind the chunks still reading it"""
    name, fused = "ragged5", True
    p = problem(name)
    l1, l2 = [0, 3], [1, 4]
    with Yardstick(name, fused, "fd_kp") as yard:
        ref1 = yard.mixed(l1, l1)
    with Yardstick(name, fused, "cols") as yard:
        refA, ref2 = yard.mixed(None, None), yard.mixed(l2, l2)
    with ss.engine(p, fused) as e:
        ss.setup(e, p)
        in1 = listed_inputs(e, p, name, "fd_kp", l1, l1)
        in2 = listed_inputs(e, p, name, "cols", l2, l2)
        whole = dict(ss.pin_rows(e, ss.rows_of(p, "A")), **ss.pin_payload(e, "cols", ss.payload_of(name, p, "cols", "A")))
        outs = [Outputs(e) for _ in range(3)]
        lam = start(e, p, name, "fd_kp")
        ss.call(e, outs[0], 3, lam, p["eps"], upload_traj=l1, **in1)
        ss.call(e, outs[1], 3, lam, p["eps"], **whole)
        ss.call(e, outs[2], 3, lam, p["eps"], upload_traj=l2, **in2)
        e.sync()
        check(outs[0], ref1, what="records, listed")
        check(outs[1], refA, what="columns, whole")
        check(outs[2], ref2, what="columns, listed")
