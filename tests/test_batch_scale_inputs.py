"""CPU checks of the inputs of tests/test_gpu_batch_scale.py (built by tests/_batch_scale.py): the list counts of the placement table,
B pairwise distinct trajectories and references in every problem, ragged lists where the lists are this suite's to choose, the
oracle's status (0 for at least 99 % of the trajectories of every problem), and the subset lists.  No GPU: n_simd is the MI355X's
1024 here."""
import numpy as np
import pytest

import _batch_scale as BS
import _shape_run as R
import _shapes as S
from trajoptkp_amd import synth

B1 = BS.N_SIMD + 1
BOUND = BS.bound_cases(BS.N_SIMD)


def _status_and_distinct(p, refs):
    bad = BS.distinct(p, refs)
    assert bad <= p["batch"] // 100, (bad, p["batch"])
    return bad


# ---- section 1a -----------------------------------------------------------------------------------------------------------------------
def test_placement_shapes_have_the_list_counts_of_the_table():
    assert [dof * B for dof, B in BS.KP_SHAPES] == list(BS.KP_LISTS) == [1022, 1024, 1026, 2050, 1029, 2051, 1054, 1056]
    assert BS.KP_HORIZONS == (5, 64, 65, 130) and len(BS.KP_METHODS) == 4
    # per = ceil(lists / 1024) of k_kp_scan: 1 up to 1024 lists, 2 above, 3 above 2048; no count above 1024 is a multiple of its per
    per = [-(-n // 1024) for n in BS.KP_LISTS]
    assert per == [1, 1, 2, 3, 2, 3, 2, 2] and [n % q for n, q in zip(BS.KP_LISTS, per)] == [0, 0, 0, 1, 1, 2, 0, 0]
    for dof, B in BS.KP_SHAPES:
        kw = BS.kp_context(dof)
        flags = S.FLAG_GENERIC if kw["generic"] else 0
        assert S.select_variants(dof, kw["m"], kw["nr"], 130, 6, B, flags) is not None, (dof, B)
    assert [kw["generic"] for kw in map(BS.kp_context, (2, 7, 31, 33))] == [False, False, False, True]
    for dof, B in BS.KP_DROPPED:                         # dof = 64: the generic context is refused at creation, whatever m
        assert BS.kp_context(dof)["generic"] and dof * B == 1088
        assert all(S.select_variants(dof, m, 3, 5, 6, B, S.FLAG_GENERIC) is None for m in range(1, 8))


@pytest.mark.parametrize("dof,B", BS.KP_SHAPES, ids=[f"d{d}b{b}" for d, b in BS.KP_SHAPES])
def test_placement_inputs_are_distinct_and_ragged(dof, B):
    for T in BS.KP_HORIZONS:
        X = BS.kp_states(dof, B, T)
        assert len(np.unique(X.reshape(B, -1), axis=0)) == B
        for method in BS.KP_METHODS:
            offs, times = BS.kp_reference(method, dof, B, T)
            assert len(offs) == dof * B + 1 and offs[-1] == len(times)
            lengths = np.diff(offs)
            if method == "set_interval":
                assert len(np.unique(lengths)) == 1
            elif T >= 64:
                assert BS.ragged_fraction(lengths) >= 0.9, (method, T, BS.ragged_fraction(lengths))
                placed = {times[offs[b * dof]:offs[(b + 1) * dof]].tobytes() + lengths[b * dof:(b + 1) * dof].tobytes() for b in range(B)}
                assert len(placed) == B, (method, T, "two trajectories with the same lists")
            else:
                assert len(np.unique(lengths)) > 1, (method, T)


# ---- section 1b -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", list(BS.FEED_METHODS))
@pytest.mark.parametrize("dof,B", list(BS.FEED_SHAPES), ids=[f"d{d}b{b}" for d, b in BS.FEED_SHAPES])
def test_fed_problems(dof, B, method):
    p, X, min_N, max_N, thr = BS.feed_problem(dof, B, method)
    assert p["batch"] == B and p["T"] == 24 and len(np.unique(X.reshape(B, -1), axis=0)) == B
    assert BS.ragged_fraction(BS.list_lengths(p["kp_rows"], dof, p["T"])) >= 0.9
    assert _status_and_distinct(p, BS.references(p)) == 0


# ---- section 1c -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [0, B1 // 2, B1 - 1, None])
def test_uniform_problems_differ_in_one_list(odd):
    p = BS.uniform_problem(B1, odd)
    lengths = BS.list_lengths(p["kp_rows"], 7, BS.UNI_T).reshape(B1, 7)
    want = np.full((B1, 7), 7)
    if odd is not None:
        want[odd, 6] = 8
    assert np.array_equal(lengths, want)
    assert _status_and_distinct(p, BS.references(p)) == 0


def test_long_uniform_problem_differs_beyond_the_in_list_stride():
    for odd in (True, False):
        p = BS.long_uniform_problem(odd)
        offs, times = BS.rows_to_dof_csr(p["kp_rows"], 7, BS.LONG_T)
        lists = times.reshape(BS.LONG_B * 7, -1)
        assert lists.shape[1] == 299 > 256
        differs = np.argwhere(lists != lists[0])
        assert differs.tolist() == ([[2 * 7 + 6, 290]] if odd else [])
        assert _status_and_distinct(p, BS.references(p)) == 0


# ---- section 2 ------------------------------------------------------------------------------------------------------------------------
def test_bound_cases_cover_the_batch_cases_and_the_pairs():
    n = BS.N_SIMD
    base = S.batch_cases(n)
    assert all(c["T"] == 12 for c in BOUND)
    for c in base:                                      # every shape of the table; the fused ones with both kinds of r_x
        twins = [d for d in BOUND if d["why"] == "batch" and all(d[k] == c[k] for k in ("dof", "m", "nr", "batch", "flags", "n_alpha"))]
        assert sorted(d["rx_const"] for d in twins) == ([False, True] if c["flags"] & S.FLAG_FUSED else [False]), c
    assert sum(c["why"] == "batch" and not c["flags"] and c["batch"] == n + 1 and c["m"] > 4 and c["dof"] in (2, 4) for c in BOUND) == 2
    assert sorted(c["batch"] for c in BOUND if c["dof"] == 12) == [n // 4, n // 4 + 1]
    assert sorted((c["batch"], c["rx_const"]) for c in BOUND if c["why"] == "pair") == [(n // 2, False), (n // 2, True), (n // 2 + 1, False), (n // 2 + 1, True)]
    eight = [c for c in BOUND if c["n_alpha"] == 8]
    assert len(eight) == 1 and eight[0]["batch"] == n + 1 and eight[0]["rx_const"] and all(c["n_alpha"] == 6 for c in BOUND if c is not eight[0])
    for c in BOUND:                                     # the pairs run below the bound, one wave above it
        d = S.dispatch(c["dof"], c["m"], c["nr"], c["T"], c["n_alpha"], c["batch"], n, c["flags"], c["env"], c["rx_const"], True, True)
        if c["why"] == "pair":
            assert (":pairh:" in d["launch"][0]) == (c["batch"] == n // 2) and (":w1:" in d["launch"][0]) == (c["batch"] == n // 2 + 1)


@pytest.mark.parametrize("i", range(len(BOUND)), ids=[R._case_id(c) for c in BOUND])
def test_bound_problems(i):
    c = BOUND[i]
    p = BS.bound_problem(c)
    assert p["batch"] == c["batch"]
    assert _status_and_distinct(p, BS.references(p, c["n_alpha"])) == 0


# ---- section 3 ------------------------------------------------------------------------------------------------------------------------
def test_subset_lists():
    lists = BS.listed_lists(B1)
    assert list(lists) == ["third", "half", "all_but_one", "third_from_2"]
    for name, who in lists.items():
        assert all(a < b for a, b in zip(who, who[1:])) and who[0] == 0 and who[-1] == B1 - 1, name
    assert len(lists["half"]) == B1 // 2 and len(lists["all_but_one"]) == B1 - 1
    assert set(range(0, B1, 3)) <= set(lists["third"]) and len(lists["third"]) <= B1 // 3 + 2
    assert len({tuple(w) for w in lists.values()}) == 4
    gaps = np.diff(lists["half"])                       # scattered: runs and holes of several lengths
    assert len(np.unique(gaps)) >= 4 and np.count_nonzero(gaps == 1) > 50


@pytest.mark.parametrize("name", [None, "third", "half", "all_but_one"])
def test_listed_problems(name):
    p0 = BS.listed_base(B1)
    p = p0 if name is None else BS.listed_regenerated(B1, name)
    who = [] if name is None else BS.listed_lists(B1)[name]
    assert BS.ragged_fraction(BS.list_lengths(p["kp_rows"], 7, BS.LISTED_T)) >= 0.9
    listed = np.isin(np.arange(B1), who)
    lam = np.where(listed, BS.listed_lambdas(B1, 1), BS.listed_lambdas(B1, 0))
    refs = BS.references(p, lam=lam)
    assert _status_and_distinct(p, refs) == 0
    if name is None:                                    # the oracle on columns (the streamed test's anchor) is the oracle on the jobs
        on_cols = BS.references_on_columns(p, p, synth.kp_columns(p), lam)
        for o, c in zip(refs, on_cols):
            assert c["status"] == 0 and max(R._rel(c[k], o[k]) for k in ("K", "k", "cost_pred")) <= 1e-12
    for b in range(B1):                                 # the listed trajectories are new in every input, the others keep every byte
        same_rows = all(np.array_equal(x, y) for x, y in zip(p["kp_rows"][b], p0["kp_rows"][b]))
        same_data = all(np.array_equal(p[k][b], p0[k][b]) for k in ("r", "r_x", "u_nom"))
        assert (same_rows, same_data) == ((not listed[b],) * 2), (name, b)
    q = BS.sub(p, who) if who else None
    if q is not None:
        assert q["batch"] == len(who) and np.array_equal(q["r"], p["r"][who]) and len(q["job_b"]) == np.count_nonzero(listed[p["job_b"]])
