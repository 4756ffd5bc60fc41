"""Shared by tests/test_gpu_streamed_sweeps.py: the cases of kpilqr_iterate_streamed5 with sweep_traj, the call itself, and its yardstick.

Shapes, data sets A / B, sentinel-guarded outputs and the pinning helpers are those of tests/_streamed_subset.py and
tests/test_gpu_streamed_columns_f32.py (imported, not copied).

The yardstick is the EXPLICIT route on a second context that starts from the same resident state (data set A swept whole):
  1. kpilqr_update_keypoints for the upload list (the same lists again, or the test's new ones: their ranges are then pending)
  2. the _partial uploads of data set B for the upload list
  3. kpilqr_iterate_partial(sweep list, compact lambdas)
  4. the device buffers read back (kpilqr_download_gains, KPILQR_BUF_*)
The wave forms of a fused context are forced by the diagnostic switches, as tests/_partial_sweeps.py forces them, so the form does not
depend on the length of a chunk's slice of the list and bit equality is a fair demand."""
import numpy as np

import _streamed_subset as ss
from _streamed_subset import CONTEXTS, IDS, KINDS, Outputs, cast, chunk_counts, engine, problem, same, setup    # noqa: F401

ONE_WAVE = {"KPILQR_FUSED_WAVES": "1", "KPILQR_FUSED_FWD_WAVES": "1"}
PAIR = {"KPILQR_FUSED_WAVES": "5", "KPILQR_FUSED_FWD_WAVES": "4"}
PAIR_TRIPLE = {"KPILQR_FUSED_WAVES": "5", "KPILQR_FUSED_FWD_WAVES": "3"}          # per-DoF lists: the triple is the pair's form for them
# form: (environment, what kpilqr_last_launch(backward) has to contain, ... (forward))
FORMS = {"one_wave": (ONE_WAVE, ":w1:kpc:", ":w1:"), "pair": (PAIR, ":pairh:kpc:", ":pair:"), "pair_triple": (PAIR_TRIPLE, ":pairh:kpc:", ":triple:"),
         "family": ({}, "", "")}
# first | last | straddling a chunk boundary (three chunks) | with gaps | all | none
SWEEP_LISTS = {7: [[0], [6], [1, 2], [1, 3, 5], list(range(7)), []], 5: [[0], [4], [0, 1], [0, 2, 4], list(range(5)), []],
               3: [[0], [2], [0, 1], [0, 2], [0, 1, 2], []]}
BUFS = ("K", "k", "cost_pred", "delta_J", "status")


def forms_of(name, fused):
    if not fused:
        return ["family"]
    return ["one_wave", "pair_triple" if name == "ragged5" else "pair"]


def set_form(monkeypatch, form):
    for key in ("KPILQR_FUSED_WAVES", "KPILQR_FUSED_FWD_WAVES"):
        monkeypatch.delenv(key, raising=False)
    for key, val in FORMS[form][0].items():                      # (read when a context is created)
        monkeypatch.setenv(key, val)


def lam_for(p, sweep, distinct):
    """the compact lambdas of a call: the problem's own, or one per listed trajectory, all different from it"""
    lam = np.full(len(sweep), float(p["lam"]))
    return lam * (1.5 + 0.25 * np.arange(len(sweep))) if distinct else lam


def buffers(e):
    """the device buffers a sweep writes, whole batch"""
    K, k = e.gains()
    return dict(K=K, k=k, **e.results())


def whole(e, p, name, kind, nchunks=3, lam=None, pd_stride=100, five=True):
    """data set A through a whole call (no list): the resident state every case starts from"""
    pl = ss.lam_of(e, p)
    if lam is not None:
        pl[:] = lam
    out = Outputs(e)
    kw = dict(ss.pin_rows(e, ss.rows_of(p, "A")), **ss.pin_payload(e, kind, ss.payload_of(name, p, kind, "A")))
    if five:
        call5(e, out, nchunks, pl, p["eps"], pd_stride=pd_stride, **kw)
    else:
        ss.call(e, out, nchunks, pl, p["eps"], pd_stride=pd_stride, **kw)
    e.sync()
    return out


def listed_inputs(e, p, name, kind, upload, which="B", every_step=(4,), pay=None):
    """the compact pinned inputs of the upload list: B's payload entries and B's rows"""
    if not len(upload):
        return {}
    pay = ss.payload_of(name, p, kind, which, every_step) if pay is None else pay
    kw = ss.pin_payload(e, kind, ss.take(pay, ss.entry_index(p, upload)))
    kw.update(ss.pin_rows(e, ss.rows_of(p, which), upload))
    return kw


def call5(e, out, nchunks, lam, eps, sweep=None, upload=None, gain=None, f32=False, pd_stride=100, **inputs):
    """Engine.iterate_streamed5 into `out`, no wait.  lam: pinned, [batch] without a sweep list, compact with one"""
    v = out.view
    e.iterate_streamed5(K=None if f32 else v["K"], k=v["k"], cost_pred=v["cost_pred"], delta_J=v["delta_J"], status=v["status"],
                        nchunks=nchunks, K32=v["K32"] if f32 else None, gain_traj=gain, lam=lam, eps=eps, upload_traj=upload,
                        sweep_traj=sweep, pd_stride=pd_stride, **inputs)


def pinned_lam(e, lam):
    a = e.pinned(max(len(lam), 1))
    a[:len(lam)] = lam
    return a


def streamed(e, p, name, kind, sweep, upload, lam, nchunks, gain=None, f32=False, pd_stride=100, inputs=None):
    """one listed call and its wait -> (outputs, buffers afterwards)"""
    out = Outputs(e)
    kw = listed_inputs(e, p, name, kind, upload) if inputs is None else inputs
    call5(e, out, nchunks, pinned_lam(e, lam), p["eps"], sweep=sweep, upload=upload if len(upload) else None, gain=gain, f32=f32,
          pd_stride=pd_stride, **kw)
    e.sync()
    return out, buffers(e)


def explicit(y, p, name, kind, sweep, upload, lam, pd_stride=100, new_rows=None, which="B", every_step=(4,), pay=None, q=None):
    """the yardstick's route on context y -> its buffers afterwards.  new_rows: {trajectory: (offs, cols)} lists that change (p: the
    problem on the OLD lists, q: on the new ones)"""
    q = p if q is None else q
    upload = [int(b) for b in upload]
    if new_rows:
        y.update_keypoints_rows(sorted(new_rows), [new_rows[b] for b in sorted(new_rows)])
        assert set(new_rows) <= set(upload)
    if upload:
        if not new_rows:
            y.update_keypoints_rows(upload, [q["kp_rows"][b] for b in upload])
        pay = ss.payload_of(name, q, kind, which, every_step) if pay is None else pay
        part = ss.take(pay, ss.entry_index(q, upload))
        if kind == "cols":
            y.upload_kp_columns_partial(upload, dict(cols=np.ascontiguousarray(part[0]).reshape(-1), entries=len(part[0])))
        elif kind == "cols32":
            y.upload_kp_columns_f32(np.ascontiguousarray(part[0]), traj=upload)
        else:
            y.upload_fd_kp_partial(upload, y.fd_kp_slab(*part, pinned=False), eps=q["eps"])
        rows = ss.rows_of(q, which)
        y.upload_residuals_partial(upload, rows["r"][upload], rows["r_x"][upload], rows["r_u"][upload])
        y.upload_nominal_partial(upload, rows["u_nom"][upload])
    if len(sweep):
        y.iterate_partial(sweep, lam, pd_stride, None)
    return buffers(y)


def launches(e):
    return [e.last_launch(w) for w in ("backward", "forward", "linearise")]


def check_compact(out, sweep, gain, want, f32=False, what=""):
    """the compact outputs of a listed call against the yardstick's buffers `want`; sentinels beyond the compact rows and around
    every output (Outputs.rows asserts them)"""
    sw = np.asarray(sweep, np.int64)
    for key in ("cost_pred", "delta_J", "status"):
        assert same(out.rows(key, len(sw)), want[key][sw]), (what, key, "compact output")
    g = np.arange(out.B) if gain is None else np.asarray(gain, np.int64)
    if f32:
        assert same(out.rows("K32", len(g)), cast(want["K"][g])), (what, "K32 is not the cast of the resident K")
        out.untouched("K")
    else:
        assert same(out.rows("K", len(g)), want["K"][g]), (what, "K")
        out.untouched("K32")
    assert same(out.rows("k", len(g)), want["k"][g]), (what, "k")


def check_buffers(after, snap, want, sweep, what=""):
    """listed rows: the yardstick's bits; everybody else's: the snapshot taken before the call"""
    B = len(snap["status"])
    sw = np.asarray(sweep, np.int64)
    rest = np.asarray([b for b in range(B) if b not in sweep], np.int64)
    for key in BUFS:
        assert same(after[key][sw], want[key][sw]), (what, key, "listed rows differ from the explicit route's")
        assert same(after[key][rest], snap[key][rest]), (what, key, "an unlisted trajectory was written")


def check_launches(e, form, want=None):
    got = launches(e)
    _, tb, tf = FORMS[form]
    assert got[0].endswith(":subset") and tb in got[0], (got, tb)
    assert got[1].endswith(":subset") and tf in got[1], (got, tf)
    assert got[2].endswith(":subset"), got
    if want is not None:
        assert got == want, (got, want)
