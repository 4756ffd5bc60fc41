"""The model behind tests/test_gpu_sequences.py, checked on the CPU so that the GPU test cannot pass vacuously.  For every committed
(kind, seed) of tests/_sequences.py:

  legality       the sequence is legal by the shadow's own rules (Shadow.illegal: the header's call order), has 40 ops and at least 10
                 observations;
  op coverage    every op class of the kind occurs across its six seeds, every documented refusal across all kinds (the tables are
                 printed: pytest -s);
  oracle status  the oracle's status is 0 for every trajectory at every observation (positive weights, lambda in [1e-2, 10]);
  sensitivity    at every observation the oracle of the shadow as it stood at the PREVIOUS observation differs from the current one, for
                 at least one trajectory, by more than 1e-6 relative in K or in the predicted costs -- unless only ops that may not change
                 a result lie in between.  A device that ignored everything since the previous observation would miss the 1e-9 bar by three
                 orders of magnitude.  The oracle is cheap at these shapes (4 x 37 steps): the check runs on all six seeds of every kind;
  no-op stretch  when only explicit stage calls, read-backs and refusals lie between two observations, the two oracle results are
                 identical: the property those ops are there to test.  No GPU."""
import collections

import numpy as np
import pytest

import _sequences as Q

NO_CHANGE = ("stage", "refuse")
CASES = [(kind, seed) for kind in Q.KINDS for seed in Q.SEEDS]


@pytest.mark.parametrize("kind,seed", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_committed_sequence(kind, seed):
    ops = Q.committed_sequence(kind, seed)
    assert len(ops) == Q.N_OPS and sum(op["op"] == "observe" for op in ops) >= Q.MIN_OBS
    sh = Q.Shadow(kind)
    prev, prev_dims, since = None, None, []
    for i, op in enumerate(ops):
        assert sh.illegal(op) is None, (i, op, sh.illegal(op))
        sh.apply(op)
        if op["op"] != "observe":
            since.append(op)
            continue
        assert not sh.missing()
        refs = sh.oracle()
        assert all(o["status"] == 0 for o in refs), (i, [o["status"] for o in refs])
        assert np.all(sh.w_run > 0) and np.all(sh.w_term > 0) and np.all((sh.lam >= 1e-2) & (sh.lam <= 10.0))
        # (a streamed observation that brings a payload or residuals changes the inputs itself)
        changed = any(o["op"] not in NO_CHANGE for o in since) or (op["how"] == "streamed" and (op.get("payload") or op.get("res")))
        if prev is not None and prev_dims == sh.dims:
            diff = max(max(Q._rel(a["K"], b["K"]), Q._rel(a["cost_pred"], b["cost_pred"])) for a, b in zip(prev, refs))
            if changed:
                assert diff > 1e-6, (i, op, since, diff)
            else:
                for a, b in zip(prev, refs):
                    for key in ("K", "k", "delta_J", "cost_pred", "U_alpha"):
                        assert np.array_equal(a[key], b[key]), (i, key, since)
        else:
            assert changed                          # the first observation of a shape follows its uploads
        prev, prev_dims, since = refs, sh.dims, []


def test_every_op_class_and_every_refusal_occurs():
    refusals = collections.Counter()
    for kind in Q.KINDS:
        seen = collections.Counter(c for seed in Q.SEEDS for op in Q.committed_sequence(kind, seed) for c in Q.op_class(op))
        print(f"{kind}: " + ", ".join(f"{c} x{seen[c]}" for c in sorted(seen)))
        missing = [c for c in Q.classes_of(kind) if not seen[c]]
        assert not missing, (kind, missing)
        refusals.update({c: n for c, n in seen.items() if c.startswith("refuse:")})
    print("refusals over all kinds: " + ", ".join(f"{c} x{n}" for c, n in sorted(refusals.items())))
    assert not [w for w in Q.REFUSALS if not refusals[f"refuse:{w}"]], refusals


def test_no_result_change_stretches_occur():
    """Per kind, at least one observation is preceded by explicit stage calls alone, and at least three follow an explicit
    differencing call (the ops after which a fused context reports another launch string)."""
    for kind in Q.KINDS:
        stretches = differenced = 0
        for seed in Q.SEEDS:
            since = []
            for op in Q.committed_sequence(kind, seed):
                if op["op"] == "observe":
                    stretches += bool(since) and all(o["op"] in NO_CHANGE for o in since)
                    differenced += any(o["op"] == "stage" and o["call"] in ("fd_difference", "fd_interpolate", "interpolate", "get_AB", "backward_stats",
                                                                            "get_union_columns", "cost_derivs") for o in since)
                    since = []
                else:
                    since.append(op)
        assert stretches >= 1 and differenced >= 3, (kind, stretches, differenced)
