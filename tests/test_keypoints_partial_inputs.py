"""CPU tests of the cases of tests/_keypoints_partial.py: the conditions that give tests/test_gpu_keypoints_partial.py its meaning,
checked with the oracle alone.  A partial placement that placed nothing, or one after which nobody's entries had to move, would
pass a comparison of lists without showing anything."""
import numpy as np
import pytest

import _keypoints_partial as C

STATE_METHODS = [m for m in C.METHODS if m != "set_interval"]
LONG_SHAPES = [s for s in C.SHAPES if s[1] >= 64]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _moves(case, traj):
    """first entry after - before, per KEPT trajectory"""
    new = C.merged(case["lists0"], case["lists1"], traj)
    return {b: C.first_entry(new, b) - C.first_entry(case["lists0"], b) for b in range(case["batch"]) if b not in traj}


@pytest.mark.parametrize("shape", C.SHAPES)
@pytest.mark.parametrize("method", C.METHODS)
def test_lists_are_canonical_and_the_subsets_are_the_four_kinds(method, shape):
    dof, T, B = shape
    c = C.list_case(method, shape)
    for lists in c["lists0"] + c["lists1"]:
        assert len(lists) == dof
        for l in lists:
            assert l[0] == 0 and l[-1] == T - 1 and np.all(np.diff(l) > 0)
    subs = {name: C.subset(name, B) for name in C.SUBSETS}
    assert subs["first"] == [0] and subs["last"] == [B - 1] and subs["all"] == list(range(B))
    a, b = subs["pair"]
    assert 0 <= a and a + 1 < b < B                                  # scattered: two runs of one trajectory


@pytest.mark.parametrize("shape", LONG_SHAPES)
@pytest.mark.parametrize("method", C.METHODS)
def test_every_listed_trajectory_gets_another_list(method, shape):
    """(At T = 2 and T = 3 there are one and two lists a DoF can have: those shapes check the staging at the horizon's ends.)"""
    c = C.list_case(method, shape)
    for b in range(c["batch"]):
        assert not _same(c["lists0"][b], c["lists1"][b]), (method, shape, b)


@pytest.mark.parametrize("method", STATE_METHODS)
def test_per_dof_lists_are_ragged(method):
    c = C.list_case(method, (3, 130, 6))
    assert any(len(set(len(l) for l in lists)) > 1 for lists in c["lists1"])


def test_kept_trajectories_move_both_ways():
    """Over the relocation cases (a kept trajectory behind a listed one) first entries move to lower offsets in one case and to
    higher ones in another, per method that reads states."""
    for method in STATE_METHODS:
        down = up = 0
        for shape in LONG_SHAPES:
            c = C.list_case(method, shape)
            for name in ("first", "pair"):
                mv = _moves(c, C.subset(name, shape[2]))
                down += any(v < 0 for v in mv.values())
                up += any(v > 0 for v in mv.values())
        assert down >= 1 and up >= 1, (method, down, up)


def test_more_than_one_block_of_listed_lists():
    c = C.many_case()
    traj = C.many_subset()
    assert len(traj) == 41 and len(traj) * c["dof"] == 287 > 256 and traj[0] == 0 and traj[-1] == c["batch"] - 1
    assert any(b - a > 1 for a, b in zip(traj, traj[1:])) and any(b - a == 1 for a, b in zip(traj, traj[1:]))      # runs and gaps
    assert all(not _same(c["lists0"][b], c["lists1"][b]) for b in traj)
    assert any(v != 0 for v in _moves(c, traj).values())


def test_the_carry_case_moves_the_payload_of_the_trajectory_behind_the_list():
    c = C.carry_case()
    traj = c["traj"]
    assert traj == [1, 2] and c["batch"] == 4 and c["T"] == 65 and c["dof"] == 7
    assert all(not _same(c["lists0"][b], c["lists1"][b]) for b in traj)
    mv = _moves(c, traj)
    assert mv[0] == 0 and mv[3] != 0, mv
    assert any(len(set(len(l) for l in lists)) > 1 for lists in c["lists1"])      # per-DoF lists: the general forms of the sweeps run
