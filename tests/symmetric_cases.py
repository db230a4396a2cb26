"""The cases shared by tests/test_symmetric_cpu.py, tests/test_gpu_symmetric.py and scripts/symmetric_tolerance.py (which records the
float32-against-float64 distances the GPU tests allow four times)."""
import json
import os

import localizability_cases as lc
import plane_to_plane_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE_FILE = os.path.join(ROOT, "profiles", "symmetric_tolerance.json")
SCENES = ("room", "corridor", "tunnel", "ellipsoid")
STARTS = lc.STARTS                      # "true": identity, "off": 0.05 rad / 0.3 m
MAX_DIST = pc.MAX_DIST
MIN_PLANE_TO_PLANE, MIN_POINT_TO_PLANE = 3, 2
CHAINS = pc.CHAINS                      # maxdist, trimmed (the fused selection), cauchy (EXT)
SUM_CASES = [(name, start, k, chain) for name in SCENES for start in ("true", "off") for k in (1, 3) for chain in CHAINS]
ELLIPSOID_ITERATIONS = 8                # the fixed-count registration on `ellipsoid`
ROOM_ITERATIONS = 12                    # the reference loops on `room` (the Differential checker stops them well before)
ROOM_TAIL = 5                           # poses behind the Differential stop whose worst error is recorded (the float32 loop's noise floor)


def recorded():
    with open(TOLERANCE_FILE) as f:
        return json.load(f)
