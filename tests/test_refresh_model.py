"""The CPU model of the running-inverse refresh and the generator that steers problems into its branches (tests/_refresh.py),
checked against themselves on every problem tests/test_gpu_refresh.py runs: every branch is reached, the unmutated model
passes the bar the GPU has to pass, and every mutation of the model -- a second-order step fewer in one bin, a give-up
threshold of 0.5, a series term left out -- misses it by a factor of ten.  No GPU."""
import collections

import numpy as np
import pytest

import _refresh as R
from oracle import pipeline

_PROBLEMS = {}
for _c in R.cases():
    for _pd in R.PD_STRIDES:
        _PROBLEMS.setdefault(R.problem_key(_c, _pd), R.case_id(dict(_c, why=_c["family"], kp_ordered=False), _pd))


def oracle_rho(p, info, pd_stride):
    """The oracle's K, k per trajectory and the worst rho they leave against the generator's recursion."""
    refs = [pipeline.run_trajectory(p, b, pd_stride=pd_stride, stages=("fd", "interp", "cost", "bwd")) for b in range(p["batch"])]
    worst = max(float(R.rho_steps(info[b], np.swapaxes(o["K"], 1, 2), o["k"]).max()) for b, o in enumerate(refs))
    return refs, worst


@pytest.mark.parametrize("key", list(_PROBLEMS), ids=list(_PROBLEMS.values()))
def test_generated_problem(key):
    task, T, family, lam, pd_stride, ragged, _ = key
    p, info = R.case_problem(key)
    assert p["rx_const"] is None and p["batch"] == 2
    # every label twice per trajectory (the first step once), on peeled and unpeeled steps apart; the distance to the thresholds
    for rec in info:
        assert rec["status"] == 0
        for pk in ((False, True) if family == "n_kink" else (False,)):
            cnt = collections.Counter(lab for t, lab in enumerate(rec["label"]) if family != "n_kink" or (t in rec["peeled"]) == pk)
            for lab, _ in R.bins(family, pk):
                assert cnt[lab] >= 2, (lab, pk, cnt)
        cnt = collections.Counter(rec["label"])
        for lab in R.family_labels(family, pd_stride, T):
            assert cnt[lab] >= (1 if lab == "ldl_first" else 2), (lab, cnt)
        for t in range(T):
            e = rec["e"][t]
            if np.isfinite(e):
                for th in R.thresholds(family):         # 1.25 from every threshold but the one its target sits right under
                    assert max(e / th, th / e) >= R.min_distance(rec["target"][T - 1 - t], th), (t, e, th)
                assert abs(e / rec["target"][T - 1 - t] - 1.0) < 1e-6, (t, e, rec["target"][T - 1 - t])
    assert R.sequences_wanted(family, pd_stride, T) <= R.sequences(family, pd_stride, info)
    assert info[0]["label"] != info[1]["label"]           # the two trajectories decide differently
    # round trip: the oracle on the returned dict
    refs, ref_rho = oracle_rho(p, info, pd_stride)
    for b, o in enumerate(refs):
        assert o["status"] == 0
        scale = max(np.max(np.abs(info[b]["K"])), 1e-300)
        assert np.max(np.abs(np.swapaxes(o["K"], 1, 2) - info[b]["K"])) <= 1e-12 * scale
    bar = R.BAR * ref_rho
    assert 1e-17 < ref_rho < 1e-13, ref_rho
    # the unmutated model is under the bar on every step; every mutation is ten times over it on some step
    signal = {}
    for b, rec in enumerate(info):
        K, k, labels = R.model_gains(family, pd_stride, rec)
        assert labels == rec["label"]
        assert R.rho_steps(rec, K, k).max() <= bar, (b, R.rho_steps(rec, K, k).max(), bar)
        for mu in R.mutations_of(family):
            Km, km, lm = R.model_gains(family, pd_stride, rec, mu)
            if mu in R.LABEL_ONLY:                      # (converges whatever it does: visible in the labels alone)
                assert lm != labels, mu
                continue
            signal[mu] = max(signal.get(mu, 0.0), float(R.rho_steps(rec, Km, km).max()))
    print(f"{_PROBLEMS[key]}: reference rho {ref_rho:.2e} bar {bar:.2e} smallest mutation signal {min(signal.values()):.2e} "
          + " ".join(f"{k}={v:.1e}" for k, v in signal.items()))
    for mu, v in signal.items():
        assert v >= 10.0 * bar, (mu, v, bar)


_INDEF = {}
for _c in R.indefinite_cases():
    _INDEF.setdefault(R.problem_key(_c, 1000, True), R.case_id(dict(_c, why=_c["family"], kp_ordered=False)))


@pytest.mark.parametrize("key", list(_INDEF), ids=list(_INDEF.values()))
def test_indefinite_problem(key):
    """One unchecked step with an indefinite Quu + lambda I: the pivoted path, a factorisation behind it, and a refresh in every bin
    on either side; the oracle finishes, and the model is under the bar on every step but the pivoted one."""
    task, T, family, lam, pd_stride, ragged, _ = key
    p, info = R.case_problem(key)
    refs = [pipeline.run_trajectory(p, b, pd_stride=pd_stride, stages=("fd", "interp", "cost", "bwd")) for b in range(2)]
    for b, rec in enumerate(info):
        lab = rec["label"]
        piv = [t for t in range(T) if lab[t] == "pivoted"]
        # (behind it: a factorisation that seeds the inverse again -- in the tiled forms the hold of the give-up first)
        assert len(piv) == 1 and lab[piv[0] - 1] == ("ldl_hold" if family in R.HOLD else "ldl_first")
        assert np.isfinite(rec["e"][piv[0] - (2 if family not in R.HOLD else R.KP_NS_HOLD + (2 if family == "plain_col" else 1))])
        assert np.min(np.linalg.eigvalsh(rec["Qreg"][piv[0]])) < -lam
        for side in (lab[:piv[0]], lab[piv[0] + 1:]):
            for name, _ in R.bins(family):
                assert name in side, (name, side)
        assert refs[b]["status"] == 0 and rec["status"] == 0
        ok = np.array([l != "pivoted" for l in lab])
        Ko = np.swapaxes(refs[b]["K"], 1, 2)
        assert np.max(np.abs(Ko - rec["K"])[ok]) <= 1e-12 * np.max(np.abs(rec["K"]))
        bar = R.BAR * float(R.rho_steps(rec, Ko, refs[b]["k"])[ok].max())
        K, k, labels = R.model_gains(family, pd_stride, rec)
        assert labels == lab and R.rho_steps(rec, K, k)[ok].max() <= bar
