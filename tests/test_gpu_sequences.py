"""GPU sequence tests: one long-lived context per (kind, seed) driven through the 40 ops of tests/_sequences.py -- key-point changes
for everybody or a subset, whole and partial uploads, explicit stage calls, kpilqr_iterate mixed with kpilqr_iterate_streamed, resizes,
documented refusals -- while a Python shadow tracks what the inputs now are.  At EVERY observation the device results must match

  1. the CPU oracle on the shadow: status equal, K, k, delta_J, predicted costs and U within 1e-9 relative (the suite's bar), and
  2. a FRESH context of the same kind and environment that is given the shadow by the shortest whole-batch route and makes the same
     observe call: np.array_equal where both contexts report the same launch strings, 1e-12 where the forms differ (raw / column store
     after an explicit fd_difference, per-DoF / union); on contexts with records also get_AB / get_cost_derivs.

What this holds in place is the validity state of Ctx (common.h: the aggregates PayloadDerived and ListsDerived) and its three
rules (kpilqr_api.cpp): an event -- payload_changed, keypoints_changed, size_buffers -- resets an aggregate as a whole, the function
that fills a store marks it, and a streamed call takes the payload-derived state back from its last chunk view.  A flag left set one
call too long makes a sweep read yesterday's linearisation, and no single-shot test reaches that state.
tests/test_sequence_model.py shows on the CPU that the sequences are legal, cover every op class and would notice a device that ignored
everything since the previous observation.  tools/sequence_fuzz.py runs the same code over uncommitted seeds.

Each test prints one line: kind, seed, observations, the distinct launch strings, the worst error per quantity."""
import collections

import pytest

import _sequences as Q

pytestmark = pytest.mark.gpu
_SEEN = collections.defaultdict(lambda: dict(seeds=set(), launches=set()))      # kind -> what its sequences have shown so far


def _line(kind, tag, st):
    worst = " ".join(f"{k}={v:.1e}" for k, v in sorted(st["worst"].items()))
    return (f"sequence {kind} {tag}: {st['observations']} observations, {len(st['launches'])} launch strings {sorted(st['launches'])}, "
            f"fresh context: {st['bit_equal']} bit-equal + {st['form_compared']} at 1e-12 (worst {st['worst_forms']:.1e}); oracle: {worst}")


@pytest.mark.parametrize("seed", Q.SEEDS)
@pytest.mark.parametrize("kind", list(Q.KINDS))
def test_sequence(kind, seed, monkeypatch):
    ops = Q.committed_sequence(kind, seed)
    st = Q.run_sequence(kind, ops, monkeypatch.setenv, monkeypatch.delenv, tag=f"{kind} seed {seed}")
    print(_line(kind, f"seed {seed}", st))
    assert st["observations"] == sum(op["op"] == "observe" for op in ops) >= Q.MIN_OBS          # none skipped
    _SEEN[kind]["seeds"].add(seed)
    _SEEN[kind]["launches"] |= st["launches"]


def test_every_fused_kind_shows_three_launch_strings():
    """Over its six seeds a fused kind runs its backward sweep in at least three forms (raw / column store, uniform / per-DoF lists,
    with and without control residuals ...): a generator that sent every observation down one form would test one set of flags.
    Holds for the kinds whose six sequences ran before this test in the same session (all of them in a run of the whole file)."""
    for kind, seen in _SEEN.items():
        if Q.Shadow(kind).fused and seen["seeds"] == set(Q.SEEDS):
            assert len(seen["launches"]) >= 3, (kind, sorted(seen["launches"]))


# ---- reduced sequences of the bugs the random ones found ----------------------------------------------------------------------------
REGRESSIONS = {
    # A context with step records, a whole payload through an ordinary upload call, then kpilqr_iterate_streamed WITHOUT a payload: the
    # chunks ran k_interpolate alone, between the key-point columns the records held from the payload BEFORE (the first observation's) --
    # nothing had written the new payload's columns there.  Fixed in kpilqr_iterate_streamed (rec_synced, kpilqr_api.cpp): the
    # resident payload is written into the records first when no call has done so since it arrived.  Found by reading the code for the
    # model (the header: "NULL inputs keep what is resident"); the fused contexts always re-differenced.
    "streamed_without_payload_after_an_ordinary_upload": ("records_t1", [
        dict(op="set_keypoints", how="bisect", seed=1), dict(op="upload_payload", kind="fd_kp", seed=2),
        dict(op="upload_residuals", what="r+rx", seed=3), dict(op="weights", seed=4), dict(op="nominal", seed=5),
        dict(op="observe", how="iterate", gains="all", seed=6),
        dict(op="upload_payload", kind="fd_kp", seed=7, same_kp=True),
        dict(op="observe", how="streamed", nchunks=3, payload=None, res=None, gains="all", seed=8),
        dict(op="upload_payload", kind="jobs", seed=9, same_kp=True),
        dict(op="observe", how="streamed", nchunks=2, payload=None, res=None, gains="all", seed=10),
        dict(op="update_keypoints", subset="pair", seed=11), dict(op="upload_payload", kind="cols", seed=12),
        dict(op="update_keypoints", subset="first", seed=13), dict(op="upload_payload_partial", seed=14),
        dict(op="observe", how="streamed", nchunks=1, payload=None, res=None, gains="all", seed=15),
    ]),
    # A union context whose slope store exists from earlier, SHORTER lists (kpilqr_backward_stats sizes one whatever the lists are, a
    # streamed call does for per-DoF lists), then kpilqr_update_keypoints makes the uniform batch ragged and longer, a key-point ordered
    # payload arrives and the first sweep takes the union route: difference_to_kpc skipped ensure_kps there (the union sweeps walk no
    # slope store) but k_fd_kp_difference wrote the slopes of every entry because a store existed -- past its end, into whatever lay
    # behind it.  The fuzz sweep saw it as KPILQR_ERR_HIP "key-point union: implausible count read back" from kpilqr_backward (the
    # counts' buffer had been written over).  Fixed: the kernel writes slopes only for a caller that has sized the store
    # (launch_fd_kp_difference's with_slopes, kpilqr_api.cpp difference_to_kpc).
    "union_route_behind_a_slope_store_of_shorter_lists": ("fused_union", [
        dict(op="set_keypoints", how="ends", seed=1), dict(op="upload_payload", kind="fd_kp", seed=2),
        dict(op="upload_residuals", what="r+rx", seed=3), dict(op="weights", seed=4), dict(op="nominal", seed=5),
        dict(op="observe", how="iterate", gains="all", seed=6),
        dict(op="stage", call="backward_stats"),
        dict(op="update_keypoints", subset="first", seed=7), dict(op="upload_payload", kind="fd_kp", seed=8, same_kp=False),
        dict(op="observe", how="staged", gains="all", seed=9),
        dict(op="update_keypoints", subset="pair", seed=10), dict(op="upload_payload_partial", seed=11),
        dict(op="observe", how="iterate", gains="f32", seed=12),
        dict(op="stage", call="fd_difference"),
        dict(op="observe", how="streamed", nchunks=3, payload=None, res=None, gains="all", seed=13),
    ]),
}
# ---- reduced sequences that pin how the validity state travels ("Who says what is still valid") ---------------------------
# The payload-derived state of the LAST chunk view is what the context holds after kpilqr_iterate_streamed: a column payload that
# arrives in 3 chunks (per-DoF lists: every chunk makes the slopes of its own entries), then kpilqr_iterate on what is resident (the
# column store has to count as valid: the payload cannot be differenced again), then a streamed call without a payload.
REGRESSIONS["streamed_column_payload_then_sweeps_on_what_is_resident"] = ("fused", [
    dict(op="set_keypoints", how="bisect", seed=1), dict(op="upload_payload", kind="fd_kp", seed=2),
    dict(op="upload_residuals", what="r+rx", seed=3), dict(op="weights", seed=4), dict(op="nominal", seed=5),
    dict(op="observe", how="iterate", gains="all", seed=6),
    dict(op="observe", how="streamed", nchunks=3, payload="cols", res=None, gains="all", seed=7),
    dict(op="observe", how="iterate", gains="all", seed=8),
    dict(op="observe", how="streamed", nchunks=2, payload=None, res=None, gains="all", seed=9),
])
# rec_synced is set by the functions that write the records (records_from_payload, linearise) and cleared by a new payload: the
# records of a fused context appear on demand behind kpilqr_fd_difference, an ordinary upload makes them stale, kpilqr_get_AB has
# them written again, and the sweeps see the new payload.  The same calls on a context that always has records.
_RECORDS_ON_DEMAND = [
    dict(op="set_keypoints", how="bisect", seed=1), dict(op="upload_payload", kind="fd_kp", seed=2),
    dict(op="upload_residuals", what="r+rx", seed=3), dict(op="weights", seed=4), dict(op="nominal", seed=5),
    dict(op="stage", call="fd_difference"), dict(op="stage", call="interpolate"),
    dict(op="upload_payload", kind="cols", seed=6, same_kp=True),
    dict(op="stage", call="get_AB"),
    dict(op="observe", how="iterate", gains="all", seed=7),
]
REGRESSIONS["records_on_demand_then_an_ordinary_upload"] = ("fused", _RECORDS_ON_DEMAND)
REGRESSIONS["records_on_demand_then_an_ordinary_upload_t1"] = ("records_t1", _RECORDS_ON_DEMAND)
REGRESSIONS["streamed_without_payload_after_an_ordinary_upload_tiled"] = ("records_tiled", REGRESSIONS["streamed_without_payload_after_an_ordinary_upload"][1])


@pytest.mark.parametrize("name", list(REGRESSIONS))
def test_reduced_sequence(name, monkeypatch):
    kind, ops = REGRESSIONS[name]
    st = Q.run_sequence(kind, ops, monkeypatch.setenv, monkeypatch.delenv, tag=name)
    print(_line(kind, name, st))
    assert st["observations"] == sum(op["op"] == "observe" for op in ops)
