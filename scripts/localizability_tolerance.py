"""Measures how far the device's constrained step lies from the float64 restatement evaluated on the same sums, over the step-parity
cases of tests/test_gpu_localizability.py, and records it: the test allows four times the recorded figure.

    python scripts/localizability_tolerance.py [--out profiles/localizability_tolerance.json]

The device works in double and rounds x once to float; angle_axis_T then builds the step in float.  A figure above 1e-5 is a defect."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localizability_tolerance.json"))
    a = ap.parse_args()
    import norlab_icp_mapper_amd as amd
    import localizability_cases as lc
    cases = {}
    for name, four, start in lc.STEP_CASES:
        r = lc.step_case(amd, name, four, start)
        cases[f"{name}/{'4dof' if four else '6dof'}/{start}"] = dict(rel_x=r["rel_x"], n_degenerate=int(r["loc"]["n_degenerate"]),
                                                                    step_norm=float((r["ref"]["y"] ** 2).sum() ** 0.5))
        print(name, four, start, cases[f"{name}/{'4dof' if four else '6dof'}/{start}"], flush=True)
    res = dict(max_rel_x=max(c["rel_x"] for c in cases.values()), quantity="|y_dev - y_ref| / |y_ref|, y = (omega L, t + omega x c)", cases=cases)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(max_rel_x=res["max_rel_x"])))


if __name__ == "__main__":
    main()
