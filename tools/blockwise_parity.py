"""The figures of profiles/blockwise_parity.txt.  (GPU box)   python tools/blockwise_parity.py [graded] [shapes] [fuzz]

Runs the graded cases of tests/test_gpu_blockwise.py (and, on request, the plain problems of tests/test_gpu_shapes.py and the
fuzz sweep of tests/test_gpu_fuzz.py) on the GPU and sets every trajectory against the extended-precision reference block by
block (tests/_blockwise.py).  Nothing is asserted: per kernel family and block family it prints the smallest block exercised
relative to max|K| (or max|k|, ...), the bar, the worst GPU error with its share of its own trajectory's bar, and the oracle's
own error; every block over its bar is listed."""
import os
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import _blockwise as BW
import _fuzz
import _shape_run as R
import _shapes as S
import pytest
from trajoptkp_amd import synth


def _smallest(ref):
    out = {}
    for f, (x, axes) in BW._family_arrays(ref).items():
        size = np.atleast_1d(np.max(np.abs(x), axis=axes) if axes else np.abs(x)).astype(float)
        out[f] = float(size[size > 0].min() / size.max()) if np.any(size > 0) else 1.0
    return out


class Table:
    def __init__(self):
        self.rows, self.over, self.n = {}, [], 0

    def add(self, fam, tag, launch, got, bb):
        self.n += 1
        errs = BW.block_errors(got, bb["ref"])
        small = _smallest(bb["ref"])
        for f in BW.FAMILIES:
            r = self.rows.setdefault((fam, f), dict(small=1.0, bar_lo=1.0, bar_hi=0.0, gpu=0.0, share=0.0, own=0.0, zero=0, zero_abs=0.0, at=""))
            share = errs[f] / bb["bar"][f]
            if share > r["share"]:
                r["at"] = tag
            r.update(small=min(r["small"], small[f]), bar_lo=min(r["bar_lo"], bb["bar"][f]), bar_hi=max(r["bar_hi"], bb["bar"][f]),
                     gpu=max(r["gpu"], errs[f]), share=max(r["share"], share), own=max(r["own"], bb["own"]["oracle"][f], bb["own"]["np"][f]),
                     zero=r["zero"] + errs[f + ":zero"], zero_abs=max(r["zero_abs"], errs[f + ":zero_abs"]))
        bad = BW.violations(errs, bb["bar"])
        if bad:
            self.over.append((tag, launch, bad, {f: bb["own"]["oracle"][f] for f in BW.FAMILIES}))

    def show(self, title):
        print(f"== {title}: {self.n} trajectories")
        print(f"{'kernel family':14s} {'blocks':7s} {'smallest':>9s} {'bar (lowest .. highest)':>25s} {'worst GPU':>10s} {'share':>6s} {'CPU own':>9s} {'zero blocks':>11s} {'abs there':>9s}  worst share at")
        for (fam, f), r in sorted(self.rows.items()):
            print(f"{fam:14s} {f:7s} {r['small']:9.1e} {r['bar_lo']:12.1e} .. {r['bar_hi']:8.1e} {r['gpu']:10.1e} {r['share']:6.2f} {r['own']:9.1e} "
                  f"{r['zero']:11d} {r['zero_abs']:9.1e}  {r['at']}")
        print(f"   blocks over their bar: {len(self.over)}")
        for o in self.over:
            print("   OVER", o)
        sys.stdout.flush()


def _family(launch):
    b = launch[0]
    return ("fused" if "fused" in b else "one_tile" if b.startswith("mfma_f64_t1") else "tiled" if "tiled" in b else "wide" if "wide" in b
            else "generic")


def run_cases(cases, graded, title):
    mp = pytest.MonkeyPatch()
    n_simd = R._n_simd()
    tab = Table()
    for c in cases:
        c = dict(c, batch=n_simd + 1) if c["batch"] > 3 else c
        if graded:
            base, p = BW.problem(c)
        else:
            base = p = R._problem(c)
        try:
            g = R._run(c, p, mp, kp_ordered=bool(c["flags"] & S.FLAG_FUSED) and (c["dof"] + c["nr"]) % 2 == 1)
        finally:
            mp.undo()
        nb = base["batch"]
        for b in (range(nb) if p["batch"] == nb else (0, p["batch"] // 2, p["batch"] - 1)):
            bb = BW.bars(base, b % nb, n_alpha=c["n_alpha"])
            if bb["status"] != 0 or g["status"][b] != 0:
                continue
            tab.add(_family(g["launch"]), f"{R._case_id(c)}[{b}]", g["launch"], BW.gpu_result(g, b), bb)
    tab.show(title)


def run_fuzz():
    from oracle import oracle as orc
    from trajoptkp_amd import Engine
    rng = np.random.default_rng(20261004)
    tab = Table()
    for case in range(220):
        c = _fuzz.draw_case(rng, case)
        saved = {key: os.environ.get(key) for key in _fuzz.ENV_KEYS}
        for key in _fuzz.ENV_KEYS:
            os.environ.pop(key, None)
        if c["form"] == "one":
            os.environ["KPILQR_FUSED_WAVES"] = "1"; os.environ["KPILQR_FUSED_FWD_WAVES"] = "1"
        if c["a6"]:
            os.environ["KPILQR_TILED_A6"] = c["a6"]
        T, batch, lam, pd = c["T"], c["batch"], c["lam"], c["pd"]
        if c["ragged"]:
            p = synth.make_ragged_problem(c["task"], T, c["rows"], config_id=c["config_id"], dense_residuals=c["dense_res"], one_sided_frac=c["osf"], lam=lam)
        else:
            p = synth.make_problem(task=c["task"], T=T, batch=batch, min_N=c["min_N"], dense_residuals=c["dense_res"], one_sided_frac=c["osf"], lam=lam,
                                   config_id=c["config_id"])
        with Engine(p["dof"], p["m"], T, p["nr"], batch=batch, fused=c["fused"]) as e:
            synth.upload(e, p, kp_ordered=c["payload"] != "jobs", rx_const=c["rx_const"])
            if c["payload"] == "columns":
                e.upload_kp_columns(e.kp_columns(*synth.kp_ordered_payload(p), eps=p["eps"]))
            if c["explicit_fd"] or "fused" not in e.backward_variant:
                e.fd_difference()
            if "fused" not in e.backward_variant:
                e.interpolate()
                if not e.backward_variant.endswith("_a6"):
                    e.cost_derivs()
            st, dJ = e.backward(lam, pd)
            K, k = e.gains()
            cost, U = e.forward_linear(orc.alphas(6), want_U=True)
            launch = (e.last_launch("backward"), e.last_launch("forward"))
        for key, val in saved.items():
            if val is None: os.environ.pop(key, None)
            else: os.environ[key] = val
        for b in range(batch):
            bb = BW.bars(p, b, lam, pd_stride=pd)
            if bb["status"] != 0 or st[b] != 0:
                continue
            tab.add(_family(launch), f"fuzz {case} {c['task']} T={T} lam={lam:.1e} pd={pd}[{b}]", launch,
                    dict(K=K[b], k=k[b], U_alpha=U[b], cost_pred=cost[b]), bb)
    tab.show("the fuzz sweep of tests/test_gpu_fuzz.py (seed 20261004, 220 cases), synth's own problems")


def main():
    what = sys.argv[1:] or ["graded"]
    if "graded" in what:
        run_cases(BW.cases(1024), True, "graded problems (tests/test_gpu_blockwise.py)")
    if "shapes" in what:
        run_cases([c for c in S.cases(1024) if c["why"] != "refused"], False, "the shape suite's own problems (tests/test_gpu_shapes.py)")
    if "fuzz" in what:
        run_fuzz()


if __name__ == "__main__":
    main()
