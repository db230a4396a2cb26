#!/usr/bin/env python
"""Measure what float32 arithmetic costs the voxel pose score (include/icpmi.h: icpmi_voxel_score_poses) on the cases of
tests/voxel_score_cases.py, and record it in profiles/voxel_score_tolerance.json: per case the relative distance of the float32
restatement (tests/voxel_score_reference.py: score32) from the float64 score on the same pairs, for likelihood and sum_maha.
tests/test_gpu_voxel_score.py allows the device four times these; under them lies a floor for the likelihood, derived from the documented
error bound of the device's expf (1 ULP: every term is positive, so the sum is off by at most 2 units of float32 roundoff of itself).
Pure numpy: no GPU, no library -- the tolerance never comes from the device's own output.

    python scripts/voxel_score_tolerance.py [--check]      (--check: measure, compare with the record, write nothing)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import voxel_score_cases as vsc  # noqa: E402
import voxel_score_reference as sr  # noqa: E402


def measure():
    rel = {}
    for size in vsc.SIZES:
        for pose in vsc.POSES:
            for n in vsc.N_VALUES:
                r64, r32 = vsc.references(size, pose, n)
                assert r64["pairs"] == r32["pairs"]
                rel[vsc.case_key(size, pose, n)] = dict(pairs=r64["pairs"], likelihood=sr.rel(r32["likelihood"], r64["likelihood"]),
                                                        sum_maha=sr.rel(r32["sum_maha"], r64["sum_maha"]))
    ranking = {}
    for (size, k), _ in vsc.PROTOTYPE.items():
        L = vsc.ranking_case(size, k)
        o = sorted(range(L.size), key=lambda i: (-L[i], i))
        ranking[f"{size}/{k}"] = dict(best=int(o[0]), best_likelihood_per_point=float(L[o[0]]), second_likelihood_per_point=float(L[o[1]]))
    return dict(rel=rel, ranking=ranking, expf_ulp_bound=vsc.EXPF_ULP_BOUND, likelihood_floor_units=vsc.LIKELIHOOD_FLOOR_UNITS, roundoff=vsc.U,
                margin=vsc.MARGIN)


def main():
    got = measure()
    if "--check" in sys.argv:
        print(json.dumps(dict(measured=got, recorded=vsc.recorded()), indent=1))
        return
    got["note"] = ("rel: |float32 restatement - float64| / |float64| of likelihood and sum_maha per case size/pose/n of tests/voxel_score_cases.py "
                   "(0 where the case has no pair); ranking: the float64 likelihood per point of the best and the second-best of the 125 "
                   "candidates; the GPU test allows max(margin x rel, likelihood_floor_units x roundoff) for the likelihood and margin x rel for "
                   "sum_maha; likelihood_floor_units = 2 x expf_ulp_bound, the documented bound of the device's expf in ULP")
    with open(vsc.TOLERANCE_FILE, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print(json.dumps(got["ranking"], indent=1))


if __name__ == "__main__":
    main()
