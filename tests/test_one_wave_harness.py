"""The checks of tests/_one_wave_backward.py checked (CPU, the oracle alone): results built from the oracle's own outputs pass
assert_oracle, and every perturbation of 2 x RTOL -- of K, one element of k, delta_J, one predicted cost, a status, the same in a
listed row -- fails it (2 x, not 1 x: a figure equal to the bar does not decide the test); assert_form on made-up launch strings;
sweep_env's environment inside the block, after it and after an exception.  hopper (12,3), T = 3, key-points every step, two
trajectories."""
import copy
import os

import numpy as np
import pytest

import _one_wave_backward as H

CASE = ("hopper", 3, 1, False)
BATCH = 2
EPS = 2.0 * H.RTOL


@pytest.fixture
def refs():
    return H.reference(*CASE, batch=BATCH)


def oracle_results(refs):
    """what run() returns, from the oracle's own outputs (copies: the cached runs stay as they are)"""
    got = {n: np.stack([np.array(o[n], float) for o in refs]) for n in ("K", "k", "delta_J", "cost_pred")}
    return dict(got, status=np.array([o["status"] for o in refs]))


def scale_K(g, b): g["K"][b] *= 1.0 + EPS
def scale_delta_J(g, b): g["delta_J"][b] *= 1.0 + EPS
def fail_status(g, b): g["status"][b] = 1


def move_one_k(g, b):
    g["k"][b].flat[np.argmin(np.abs(g["k"][b]))] += EPS * np.max(np.abs(g["k"][b]))


def scale_one_cost(g, b):
    g["cost_pred"][b].flat[np.argmax(np.abs(g["cost_pred"][b]))] *= 1.0 + EPS


PERTURBATIONS = [scale_K, move_one_k, scale_delta_J, scale_one_cost, fail_status]


def test_oracle_outputs_pass_and_the_worst_figures_come_back(refs):
    assert all(o["status"] == 0 for o in refs)
    worst = H.assert_oracle(oracle_results(refs), refs, "oracle", quiet=True)
    assert worst == dict(K=0.0, k=0.0, delta_J=0.0, cost_pred=0.0)
    got = oracle_results(refs)
    got["K"][1] *= 1.0 + 0.25 * H.RTOL          # below the bar: passes, and is reported
    worst = H.assert_oracle(got, refs, "oracle", quiet=True)
    assert 0.2 * H.RTOL < worst["K"] < 0.3 * H.RTOL and worst["k"] == 0.0


@pytest.mark.parametrize("b", range(BATCH))
@pytest.mark.parametrize("perturb", PERTURBATIONS, ids=lambda f: f.__name__)
def test_a_perturbation_of_twice_the_bar_fails(refs, perturb, b):
    got = oracle_results(refs)
    perturb(got, b)
    with pytest.raises(AssertionError):
        H.assert_oracle(got, refs, "perturbed", quiet=True)


@pytest.mark.parametrize("perturb", PERTURBATIONS, ids=lambda f: f.__name__)
def test_a_perturbation_in_a_listed_row_fails(refs, perturb):
    """rows: refs[i] is trajectory rows[i] of a batch of five; the unlisted rows hold nothing the check may read"""
    rows = [3, 1]
    listed = oracle_results(refs)
    got = {n: np.full((5,) + v.shape[1:], np.nan) for n, v in listed.items()}
    for n, v in listed.items():
        got[n][rows] = v
    assert H.assert_oracle(got, refs, "listed", rows=rows, quiet=True)["K"] == 0.0
    for b in rows:
        bad = copy.deepcopy(got)
        perturb(bad, b)
        with pytest.raises(AssertionError):
            H.assert_oracle(bad, refs, "listed", rows=rows, quiet=True)
    with pytest.raises(AssertionError):          # the right rows in the wrong order
        H.assert_oracle(got, refs, "listed", rows=rows[::-1], quiet=True)


def test_an_oracle_failure_is_not_a_success(refs):
    bad = [dict(o) for o in refs]
    bad[0]["status"] = 2
    got = oracle_results(bad)
    with pytest.raises(AssertionError):
        H.assert_oracle(got, bad, "both fail", quiet=True)


def test_forms_of_one_sweep_are_held_to_ftol(refs):
    a = oracle_results(refs)
    H.assert_forms_agree(a, oracle_results(refs), "same")
    H.assert_bit_identical(a, oracle_results(refs))
    b = oracle_results(refs)
    b["K"] *= 1.0 + 2.0 * H.FTOL
    with pytest.raises(AssertionError):
        H.assert_forms_agree(a, b, "K")
    with pytest.raises(AssertionError):
        H.assert_bit_identical(a, b)
    b = oracle_results(refs)
    b["status"][1] = 1
    with pytest.raises(AssertionError):
        H.assert_forms_agree(a, b, "status")


UNI = "mfma_f64_t1_fused:w1:raw:uni:x:rxc"
GEN = "mfma_f64_t1_fused:w1:raw:gen:x"


def test_assert_form():
    H.assert_form(UNI, "raw")
    H.assert_form(dict(launch=UNI), "raw", rxc=True)
    H.assert_form(UNI.replace(":raw:", ":kpc:"), "kpc", rxc=True)
    H.assert_form(GEN, "raw", rxc=False, general=True)
    for lb, payload, kw in ((UNI.replace(":w1:", ":pairh:"), "raw", {}),          # not one wave
                            (UNI, "kpc", {}),                                       # the other payload
                            (UNI, "raw", dict(general=True)),                       # uniform where the general form is asked for
                            (GEN, "raw", {}),                                       # and the other way round
                            (UNI, "raw", dict(rxc=False)),                          # a constant Jacobian where none was uploaded
                            (GEN, "raw", dict(rxc=True, general=True))):
        with pytest.raises(AssertionError):
            H.assert_form(lb, payload, **kw)


@pytest.mark.parametrize("one_wave,general", [(True, False), (True, True), (False, False)])
def test_sweep_env(monkeypatch, one_wave, general):
    monkeypatch.setenv("KPILQR_FUSED_WAVES", "2")
    monkeypatch.setenv("KPILQR_FUSED_UNI", "0")
    monkeypatch.setenv("KPILQR_FUSED_RAW", "0")
    monkeypatch.delenv("KPILQR_FUSED_FWD_WAVES", raising=False)
    before = dict(os.environ)
    want = {}
    if one_wave:
        want.update(KPILQR_FUSED_WAVES="1", KPILQR_FUSED_FWD_WAVES="1")
    if general:
        want.update(KPILQR_FUSED_UNI="0")
    with H.sweep_env(one_wave, general):
        assert {key: os.environ[key] for key in H.WAVE_KEYS if key in os.environ} == want
    assert dict(os.environ) == before
    with pytest.raises(RuntimeError):
        with H.sweep_env(one_wave, general):
            assert {key: os.environ[key] for key in H.WAVE_KEYS if key in os.environ} == want
            raise RuntimeError("inside")
    assert dict(os.environ) == before


def test_cached_calls_are_one_entry_however_they_are_spelt():
    a = H.reference(*CASE, batch=BATCH)
    assert H.reference(*CASE, 100, BATCH) is a and H.reference(*CASE, pd_stride=100, batch=BATCH, lam=0.1) is a
    assert H.reference(*CASE, 2, BATCH) is not a
    assert H.problem(*CASE, BATCH) is H.problem(*CASE, batch=BATCH, one_sided_frac=0.25)
