"""The table of profiles/clamp_parity.txt: per forward family the number of clamp cases (tests/test_gpu_clamp.py:
test_shape_clamped_matches_oracle and test_clamped_batch_boundaries), the range of the oracle's share of controls on a limit,
the fewest hits of a control on one of its limits, the fewest entries whose on-limit flag differs between the first and the last
alpha, and the worst relative error of U_alpha and cost_pred on the GPU.

Usage:  python -m pytest -m gpu tests/test_gpu_clamp.py -rA | python tools/clamp_parity.py       (one GPU: the tests print a line per case)
        python tools/clamp_parity.py --cpu                                                        (no GPU: the oracle's columns)"""
import collections
import os
import re
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]

LINE = re.compile(r"^clamp_parity (\S+) (\S+) share=(\S+) hits=(\d+) differ=(\d+) U=(\S+) cost=(\S+)")


def cpu_rows():
    import _clamp
    import _shapes as S
    from _shape_run import _case_id, _problem
    n_simd = 1024
    cases = [(c, None) for c in S.cases(n_simd) if c["why"] != "refused"] + [(c, 7) for c in S.batch_cases(n_simd) if c["batch"] == n_simd + 1]
    for c, nb in cases:
        p = _problem(c) if nb is None else _problem(dict(c, T=17), batch=nb, config_id=5)
        lin = _clamp.linearise(p)
        cond = _clamp.conditions(_clamp.activate(p, c["n_alpha"], lin), c["n_alpha"], lin)
        yield (S.case_keys(c, n_simd)[1][0], _case_id(c), cond["share"], min(cond["hits_lo"], cond["hits_hi"]), cond["differ"],
               float("nan"), float("nan"))


def log_rows(lines):
    for line in lines:
        m = LINE.match(line)
        if m:
            yield (m.group(1), m.group(2), float(m.group(3)), int(m.group(4)), int(m.group(5)), float(m.group(6)), float(m.group(7)))


def main():
    rows = list(cpu_rows() if "--cpu" in sys.argv else log_rows(sys.stdin))
    fam = collections.defaultdict(list)
    for r in rows:
        fam[r[0]].append(r)
    print("forward family | cases | oracle share on a limit (min .. max) | fewest hits per control and limit | fewest entries "
          "differing first / last alpha (n_alpha > 1) | GPU worst rel. error U_alpha | cost_pred")
    for f in sorted(fam):
        rs = fam[f]
        differ = [r[4] for r in rs if "-a1-" not in r[1]]
        print(f"{f} | {len(rs)} | {min(r[2] for r in rs):.3f} .. {max(r[2] for r in rs):.3f} | {min(r[3] for r in rs)} | {min(differ)} | "
              f"{max(r[5] for r in rs):.2e} | {max(r[6] for r in rs):.2e}")
    print(f"all | {len(rows)} | {min(r[2] for r in rows):.3f} .. {max(r[2] for r in rows):.3f} | {min(r[3] for r in rows)} | - | "
          f"{max(r[5] for r in rows):.2e} | {max(r[6] for r in rows):.2e}")


if __name__ == "__main__":
    main()
