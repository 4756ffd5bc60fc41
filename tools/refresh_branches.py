"""The table of profiles/refresh_branches.txt: for every case of tests/test_gpu_refresh.py the label counts of the generated
problem, the reference's rho, the bar, the smallest signal a mutation of the CPU model leaves, the GPU's worst rho and, for the
fused general form, the instrumented sweep's histogram against the model's.  Asserts what the tests assert.

Usage:  python tools/refresh_branches.py > profiles/refresh_branches.txt      (one GPU)
        python tools/refresh_branches.py --cpu                                (no GPU: the columns the CPU gives)"""
import collections
import contextlib
import io
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]

import _refresh as R                                    # noqa: E402
import _shapes as S                                     # noqa: E402
import numpy as np                                      # noqa: E402
from oracle import pipeline                             # noqa: E402

CPU_ONLY = "--cpu" in sys.argv
if not CPU_ONLY:
    import test_gpu_refresh as G                        # noqa: E402


def cpu_figures(c, pd_stride, indefinite):
    p, info = R.case_problem(R.problem_key(c, pd_stride, indefinite))
    fig = dict(labels=[], ref_rho=0.0, gpu_rho=float("nan"), worst="not run", hist=[], hist_model=[])
    for b, rec in enumerate(info):
        o = pipeline.run_trajectory(p, b, pd_stride=pd_stride, stages=("fd", "interp", "cost", "bwd"))
        ok = np.array([lab != "pivoted" for lab in rec["label"]])
        fig["ref_rho"] = max(fig["ref_rho"], float(R.rho_steps(rec, np.swapaxes(o["K"], 1, 2), o["k"])[ok].max()))
        fig["labels"].append({l: rec["label"].count(l) for l in sorted(set(rec["label"]))})
        if c["why"] == "fused_w1_general":
            fig["hist_model"].append(R.hist_of(rec["label"]))
    fig["bar"] = R.BAR * fig["ref_rho"]
    return fig


def mutation_signal(c, pd_stride, indefinite):
    p, info = R.case_problem(R.problem_key(c, pd_stride, indefinite))
    sig = {}
    for rec in info:
        ok = [lab != "pivoted" for lab in rec["label"]]
        for mu in R.mutations_of(c["family"]):
            if mu not in R.LABEL_ONLY:
                K, k, _ = R.model_gains(c["family"], pd_stride, rec, mu)
                sig[mu] = max(sig.get(mu, 0.0), float(R.rho_steps(rec, K, k)[ok].max()))
    return min(sig.items(), key=lambda kv: kv[1])


def main():
    saved = {k: os.environ.get(k) for k in S.ENV_KEYS}
    setenv = os.environ.__setitem__
    delenv = lambda k: os.environ.pop(k, None)
    rows = [(c, pd, False) for c in R.cases() for pd in R.PD_STRIDES] + [(c, 1000, True) for c in R.indefinite_cases()]
    worst = collections.defaultdict(lambda: dict(ref=[0.0, 1.0], bar=[0.0, 1.0], sig=1.0, gpu=0.0, n=0))
    print("case | family | labels of trajectory 0 | reference rho | bar | smallest mutation signal | GPU worst rho (trajectory, label)")
    for c, pd, indef in rows:
        sys.stdout.flush()
        if CPU_ONLY:
            fig = cpu_figures(c, pd, indef)
        else:
            with contextlib.redirect_stdout(io.StringIO()):     # (check_case prints its own line for pytest -s)
                fig = G.check_case(c, pd, setenv, delenv, indefinite=indef)
        mu, sig = mutation_signal(c, pd, indef)
        labels = " ".join(f"{k}:{v}" for k, v in fig["labels"][0].items())
        print(f"{R.case_id(c, pd)}{' indefinite' if indef else ''} | {c['family']} | {labels} | {fig['ref_rho']:.2e} | {fig['bar']:.2e} | "
              f"{sig:.2e} ({mu}) | {fig['gpu_rho']:.2e} ({fig['worst']})")
        if fig["hist_model"]:
            print(f"    histogram {fig['hist'] or 'not run'} model {fig['hist_model']}")
        w = worst[c["why"]]
        w["ref"] = [max(w["ref"][0], fig["ref_rho"]), min(w["ref"][1], fig["ref_rho"])]
        w["sig"] = min(w["sig"], sig); w["n"] += 1
        w["gpu"] = float("nan") if CPU_ONLY else max(w["gpu"], fig["gpu_rho"])      # (a column that was not run stays nan)
    print(f"\nper kernel form: cases | reference rho (min .. max) | bar ({R.BAR:g} x) | smallest mutation signal | GPU worst rho")
    for why, w in worst.items():
        print(f"{why} | {w['n']} | {w['ref'][1]:.2e} .. {w['ref'][0]:.2e} | {R.BAR * w['ref'][1]:.2e} .. {R.BAR * w['ref'][0]:.2e} | {w['sig']:.2e} | {w['gpu']:.2e}")
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


if __name__ == "__main__":
    main()
