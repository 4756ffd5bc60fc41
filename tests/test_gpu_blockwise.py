"""Every compiled kernel instantiation held to the extended-precision reference block by block (tests/_blockwise.py), on graded
problems: K per step, per (step, control row) and per (step, state column), k per step, U_alpha per (alpha, step) and the
predicted cost per alpha, each block relative to its OWN largest reference entry, against bars taken from the two CPU float64
implementations' own blockwise errors -- where the rest of the suite divides by the largest entry of the whole trajectory and
leaves a small row, column or step free to be wrong in its leading digits.  The cases (BW.cases) reach every key of
_shapes.COMPILED; each asserts the variant and launch strings the dispatch table predicts, as tests/test_gpu_shapes.py does, and
keeps that suite's global 1e-9 beside the bars.  tests/test_blockwise_model.py checks the cases' inputs and the measure without a
GPU.

What it found (profiles/blockwise_parity.txt): with the Newton-Schulz refresh of the tiled and wide backward sweeps counting its steps
from the residual's largest entry alone, 29 of these cases missed on K's (step, control row) blocks -- 2.3e-8 against a bar of 3.2e-14
(tiled col, dof 1, m 2, step 8, row 1; the oracle 6.5e-16), 4.4e-8 at T = 131 -- in rows below 1e-14 of the step's largest.  The refresh
now takes one more step where an entry of the inverse moved too far of itself for the bin's count (kp_inverse_refresh, mfma_common.h);
every case passes, the two families at 0.10 and 0.09 of that bar."""
import pytest

import _blockwise as BW
import _shapes as S
from _shape_run import RTOL, _case_id, _check_dispatch, _global_errs, _n_simd, _run

pytestmark = pytest.mark.gpu

_CASES = BW.cases(1024)


def _on_device(c, n_simd):
    """The case on this device: the batches past the `excl` bound are n_simd + 1 of ITS SIMD count."""
    return dict(c, batch=n_simd + 1) if c["batch"] > 3 else c


def test_cases_reach_every_compiled_key_on_this_device():
    n_simd = _n_simd()
    covered = set()
    for c in _CASES:
        covered.update(S.case_keys(_on_device(c, n_simd), n_simd))
    missing = [k for k in S.COMPILED if k not in covered]
    assert not missing, missing


@pytest.mark.parametrize("c", _CASES, ids=[_case_id(c) for c in _CASES])
def test_graded_case_blockwise(c, monkeypatch):
    n_simd = _n_simd()
    c = _on_device(c, n_simd)
    base, p = BW.problem(c)                               # 2 .. 3 distinct trajectories; tiled up to n_simd + 1 where the case asks
    kp_ordered = bool(c["flags"] & S.FLAG_FUSED) and (c["dof"] + c["nr"]) % 2 == 1     # both payload forms over the fused cases
    g = _run(c, p, monkeypatch, kp_ordered=kp_ordered)
    _check_dispatch(c, g, n_simd)
    nb = base["batch"]
    rows = range(nb) if p["batch"] == nb else (0, p["batch"] // 2, p["batch"] - 1)     # first, a middle and the last trajectory
    for b in rows:
        bb = BW.bars(base, b % nb, n_alpha=c["n_alpha"])
        assert g["status"][b] == bb["status"] == 0, (b, g["status"][b], bb["status"])
        errs = _global_errs(g, bb["oracle"], b)
        assert max(errs.values()) <= RTOL, (b, g["launch"], errs)
        BW.check(BW.gpu_result(g, b), base, b % nb, (_case_id(c), g["launch"]), n_alpha=c["n_alpha"])
