"""The cases shared by tests/test_plane_to_plane_cpu.py, tests/test_gpu_plane_to_plane.py and scripts/plane_to_plane_tolerance.py (which
records the float32-against-float64 distances the GPU tests allow four times)."""
import json
import os

import localizability_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE_FILE = os.path.join(ROOT, "profiles", "plane_to_plane_tolerance.json")
SCENES = ("room", "corridor", "tunnel")
STARTS = lc.STARTS                      # "true": identity, "off": 0.05 rad / 0.3 m
EPSILONS = (1e-3, 1.0)
MAX_DIST = 2.0
MIN_PLANE_TO_PLANE, OUT_MAXDIST, OUT_TRIMMED, OUT_ROBUST = 3, 1, 4, 7
# chain -> the library's outlier list and what plane_to_plane_reference.scene_pairs takes for it
CHAINS = {
    "maxdist": dict(outliers=[(OUT_MAXDIST, MAX_DIST)], reference=dict(max_dist=MAX_DIST)),
    "trimmed": dict(outliers=[(OUT_TRIMMED, 0.85)], reference=dict(max_dist=MAX_DIST, trimmed=0.85)),        # the fused selection
    "cauchy": dict(outliers=[(OUT_ROBUST, 1.0, 0 | (0 << 4) | (0 << 8), 0.0, 0.0)], reference=dict(max_dist=MAX_DIST, cauchy=1.0)),   # EXT
}
SUM_CASES = [(name, start, k, chain) for name in SCENES for start in ("true", "off") for k in (1, 3) for chain in CHAINS]


def recorded():
    with open(TOLERANCE_FILE) as f:
        return json.load(f)
