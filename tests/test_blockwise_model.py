"""The blockwise measure of tests/_blockwise.py on the CPU alone (no GPU): the graded problems of tests/test_gpu_blockwise.py meet
the conditions that make the measure bite (conditions on the inputs, read off the oracle), the two CPU float64 implementations
pass each other's bars, and the measure notices three errors that max|a - b| / max|b| at 1e-9 -- the measure of the rest of the
suite -- does not: applied to the oracle's own K, k, U_alpha, in every trajectory of every case."""
import numpy as np
import pytest

import _blockwise as BW
import _shapes as S
from _shape_run import _case_id

N_SIMD = 1024          # an MI355X (256 CUs x 4); the GPU tests read it from the device
CASES = BW.cases(N_SIMD)
SMALL = 1e-6           # a block this far below max|K| is what a global 1e-9 leaves three digits of slack in


def _trajectories(c):
    base, _ = BW.problem(c)
    return [(b, BW.bars(base, b, n_alpha=c["n_alpha"])) for b in range(base["batch"])]


def _sizes(K):
    a = np.abs(K)
    return a.max(axis=1) / a.max(), a.max(axis=2) / a.max()            # (step, control row), (step, state column) over max|K|


def test_cases_reach_every_compiled_key_and_the_listed_shapes():
    covered = set()
    for c in CASES:
        keys = S.case_keys(c, N_SIMD)
        assert keys and all(k in S.COMPILED for k in keys), c
        covered.update(keys)
    assert not [k for k in S.COMPILED if k not in covered]
    shapes = {(BW.family(c), S.tiled_nt(2 * c["dof"]), c["m"]) for c in CASES}
    assert all(("tiled", nt, m) in shapes for nt in (2, 3, 4) for m in (1, 7, 8))
    assert all(("wide", nt, m) in shapes for nt in (2, 3, 4) for m in (9, 17, 32))
    for n, m in S.T1_SHAPES:
        forms = {(bool(c["flags"] & S.FLAG_FUSED), c["batch"] > N_SIMD) for c in CASES if (2 * c["dof"], c["m"]) == (n, m) and BW.family(c) == "one_tile"}
        assert forms >= {(False, True), (True, False), (True, True)}, (n, m, forms)        # (unfused or fused, n_simd + 1 trajectories or two)
    long_families = {BW.family(c) for c in CASES if c["T"] == 131}
    assert long_families == {"one_tile", "tiled", "wide", "generic"}
    assert all(c["T"] in (17, 131) for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=[_case_id(c) for c in CASES])
def test_case_conditions_and_cpu_implementations(c):
    """Status 0 at the lambda used, at most 10 % of K's blocks exactly zero, every bar <= 1e-10; the oracle and np_pipeline within
    each other's bars whichever of the two is taken as the reference."""
    for b, bb in _trajectories(c):
        assert bb["status"] == 0, (b, bb["status"])
        rows, cols = _sizes(bb["oracle"]["K"])
        assert np.mean(rows == 0) <= 0.10 and np.mean(cols == 0) <= 0.10, (b, np.mean(rows == 0), np.mean(cols == 0))
        assert max(bb["bar"].values()) <= 1e-10, (b, bb["bar"])
        assert not BW.violations(bb["own"]["oracle"], bb["bar"]) and not BW.violations(bb["own"]["np"], bb["bar"])
        assert not BW.violations(BW.block_errors(bb["oracle"], bb["np"]), bb["bar"]), b
        assert not BW.violations(BW.block_errors(bb["np"], bb["oracle"]), bb["bar"]), b


@pytest.mark.parametrize("fam", ["one_tile", "tiled", "wide", "generic"])
def test_every_family_has_small_rows_and_columns(fam):
    """At least one trajectory of the family's table with a (step, control row) block, and one with a (step, state column) block,
    below 1e-6 of that trajectory's max|K|."""
    small_row = small_col = 0
    for c in CASES:
        if BW.family(c) != fam:
            continue
        for b, bb in _trajectories(c):
            rows, cols = _sizes(bb["oracle"]["K"])
            small_row += bool(np.any((rows > 0) & (rows < SMALL)))
            small_col += bool(np.any((cols > 0) & (cols < SMALL)))
    assert small_row >= 1 and small_col >= 1, (fam, small_row, small_col)


def _perturbed(o):
    """The three errors, each applied alone to a copy of the oracle's result: name -> (result, the array it touched)."""
    out = {}
    K, k = o["K"], o["k"]
    # 1. the smallest nonzero (step, control row) block of K times 1 + 1e-6
    rows = np.abs(K).max(axis=1)
    t, j = np.unravel_index(np.argmin(np.where(rows > 0, rows, np.inf)), rows.shape)
    Kp = K.copy(); Kp[t, :, j] *= 1.0 + 1e-6
    out["row"] = dict(o, K=Kp), "K"
    # 2. one state column of K at one step replaced by the next step's: the (step, column) where that changes K least (and changes it)
    d = np.abs(K[1:] - K[:-1]).max(axis=2)
    t, i = np.unravel_index(np.argmin(np.where(d > 0, d, np.inf)), d.shape)
    Kp = K.copy(); Kp[t, i, :] = K[t + 1, i, :]
    out["column"] = dict(o, K=Kp), "K"
    # 3. the smallest nonzero k_t times 1 + 1e-6
    ks = np.abs(k).max(axis=1)
    t = int(np.argmin(np.where(ks > 0, ks, np.inf)))
    kp = k.copy(); kp[t] *= 1.0 + 1e-6
    out["k"] = dict(o, k=kp), "k"
    return out


@pytest.mark.parametrize("c", CASES, ids=[_case_id(c) for c in CASES])
def test_measure_notices_what_the_global_one_does_not(c):
    for b, bb in _trajectories(c):
        o = {key: bb["oracle"][key] for key in ("K", "k", "U_alpha", "cost_pred")}
        assert not BW.violations(BW.block_errors(o, bb["ref"]), bb["bar"])
        for name, (got, key) in _perturbed(o).items():
            assert not np.array_equal(got[key], o[key]), (name, b)
            old = max(BW.relerr(got[x], o[x]) for x in ("K", "k", "U_alpha", "cost_pred"))
            assert old < 1e-9, (name, b, old)                                       # invisible to the measure of the rest of the suite
            assert BW.violations(BW.block_errors(got, bb["ref"]), bb["bar"]), (name, b)


def test_block_errors_on_known_arrays():
    """The arithmetic of block_errors itself: per-block relative errors, exactly-zero reference blocks held absolutely and counted."""
    T, n, m, na = 3, 4, 2, 2
    ref = dict(K=np.zeros((T, n, m)), k=np.ones((T, m)), U_alpha=np.ones((na, T, m)), cost_pred=np.array([1.0, -2.0]))
    ref["K"][0] = 1.0; ref["K"][1, :, 0] = 1e-8; ref["K"][1, 2, 1] = 1e-3            # step 2 and row 1 of step 1 (but one entry): zero
    got = {key: v.copy() for key, v in ref.items()}
    got["K"][1, 0, 0] = 1e-8 * (1 + 1e-3)                                           # a small row, wrong in its third digit
    got["K"][2, 1, 1] = 1e-12                                                       # inside an exactly zero block
    got["cost_pred"][1] = -2.0 * (1 + 1e-5)
    e = BW.block_errors(got, ref)
    assert e["K_row"] == pytest.approx(1e-3, rel=1e-6) and e["K_step"] == pytest.approx(1e-11 / 1e-3, rel=1e-3)
    assert e["K_col"] == pytest.approx(1e-3, rel=1e-6)                              # (state 0 of step 1: reference max 1e-8)
    assert e["K_step:zero"] == 1 and e["K_row:zero"] == 2 and e["K_col:zero"] == n
    assert e["K_step:zero_abs"] == pytest.approx(1e-12) and e["k_step"] == 0.0 and e["U_step"] == 0.0
    assert e["cost"] == pytest.approx(1e-5, rel=1e-6)
    bar = {f: 1e-10 for f in BW.FAMILIES}
    assert {v[0] for v in BW.violations(e, bar)} == {"K_step", "K_row", "K_col", "cost"}
    got["K"][2, 1, 1] = 1e-8                                                        # the absolute fallback: 1e-9 x max|K|
    assert "K_step:zero_abs" in {v[0] for v in BW.violations(BW.block_errors(got, ref), bar)}
