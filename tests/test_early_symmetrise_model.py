"""The CPU study behind the early symmetrisation of the uniform one-wave backward sweep (tools/early_symmetrise_error.py): V = sym(Qzz) + K'G
against V = sym(Qzz + K'G) in a numpy restatement of the recursion, at T = 64 on two seeds of every workload of the tool and every
lambda of its list.  The gate is the tool's: the gains of the two variants stay within 1e-13 of each other, a decade under the 1e-12
at which the GPU tests hold kernel forms to one another.  (The committed table, profiles/early_symmetrise.txt, is the full-size run.)"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("early_symmetrise_error", os.path.join(ROOT, "tools", "early_symmetrise_error.py"))
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)


@pytest.mark.parametrize("case", range(len(tool.CASES)), ids=[name for name, _ in tool.CASES])
def test_gate_at_T64_on_two_seeds(case):
    name, kw = tool.CASES[case]
    res = tool.study(dict(kw, T=64, batch=2))
    assert sorted(res) == sorted(tool.LAMS) == [1e-4, 1e-2, 0.1, 1.0, 10.0]
    for lam, w in res.items():
        print(f"{name} T=64 lambda={lam:g}: K {w['K']:.1e} k {w['k']:.1e} delta_J {w['delta_J']:.1e} asymmetry of V {w['asym']:.1e}")
        assert w["K"] < tool.GATE == 1e-13, (name, lam, w)
        # V of the early variant is symmetric up to the rounding of one product: far below anything a 1e-12 comparison sees
        assert w["asym"] < 1e-14, (name, lam, w)
