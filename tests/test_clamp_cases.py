"""The clamp cases of tests/test_gpu_clamp.py on the CPU oracle alone (no GPU): every case of tests/_shapes.py, with the inputs of
tests/_clamp.activate, meets the conditions under which a wrong clamp cannot hide -- 15 to 45 % of the controls on a limit, every
control on each of its two limits at least twice, a clamped set that changes with alpha -- and the cases reach every compiled
forward key.  The same cases as tests/test_gpu_shapes.py runs them never touch a limit, which is why that suite does not cover
the clamp."""
import functools

import pytest

import _clamp
import _shapes as S
from _shape_run import _case_id, _problem

N_SIMD = 1024          # an MI355X (256 CUs x 4); the GPU tests read it from the device
FORWARD_FAMILIES = ("t1_fwd", "fused_fwd", "tiled_fwd", "tiled_fwd_sc", "wide_fwd", "generic_fwd")

_CASES = [c for c in S.cases(N_SIMD) if c["why"] != "refused"]
_BATCH_CASES = [c for c in S.batch_cases(N_SIMD) if c["batch"] == N_SIMD + 1]
_ALL = [("shape", c) for c in _CASES] + [("batch", c) for c in _BATCH_CASES]
_IDS = [_case_id(c) for _, c in _ALL]


@functools.lru_cache(maxsize=None)
def _figures(i):
    """(conditions of the activated problem, conditions of the problem as test_gpu_shapes runs it) of case i, one backward pass."""
    kind, c = _ALL[i]
    # the problems of test_shape_matches_oracle / test_batch_boundaries (7 distinct trajectories, tiled there to the batch)
    p = _problem(c) if kind == "shape" else _problem(dict(c, T=17), batch=7, config_id=5)
    lin = _clamp.linearise(p)
    return _clamp.conditions(_clamp.activate(p, c["n_alpha"], lin), c["n_alpha"], lin), _clamp.conditions(p, c["n_alpha"], lin)


@pytest.mark.parametrize("i", range(len(_ALL)), ids=_IDS)
def test_activated_case_meets_the_clamp_conditions(i):
    c = _ALL[i][1]
    cond, _ = _figures(i)
    _clamp.assert_conditions(cond, c["n_alpha"], _IDS[i])
    assert cond["ran"] >= 1 and (cond["ran"] == (7 if _ALL[i][0] == "batch" else c["batch"]) or c["why"] == "long"), cond


@pytest.mark.parametrize("i", range(len(_ALL)), ids=_IDS)
def test_unactivated_case_never_clamps(i):
    _, plain = _figures(i)
    assert plain["clamped"] == 0, (_IDS[i], plain)


def test_every_compiled_forward_key_is_reached_by_a_clamp_case():
    reached = set()
    for _, c in _ALL:
        reached.update(k for k in S.case_keys(c, N_SIMD) if k[0] in FORWARD_FAMILIES)
    want = [k for k in S.COMPILED if k[0] in FORWARD_FAMILIES]
    assert {k[0] for k in want} == set(FORWARD_FAMILIES)
    assert any("plain" in k for k in want)
    missing = [k for k in want if k not in reached]
    assert not missing, missing
