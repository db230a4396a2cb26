"""The cases of tests/test_gpu_loop_weights.py, and a CPU replay of the loop on the oracle's matcher and minimiser
(tests/test_weights_reference.py evaluates the undecidable-pairs condition of every case with it before the GPU is asked)."""
import math

import numpy as np

import weights_reference as wr
from loop_driver import weights_scene

FCT = {"cauchy": 0, "welsch": 1, "sc": 2, "gm": 3, "tukey": 4, "huber": 5, "L1": 6, "student": 7}
SOFT, LARGER, READING = wr.GEN_SOFT, wr.GEN_LARGER, wr.GEN_READING


def rob(fct, tuning, scale="none", nb=0, dist="point2point", approximation=0.0):
    return (wr.ROBUST, float(tuning), FCT[fct] | ({"none": 0, "mad": 1, "berg": 2, "std": 3}[scale] << 4) | ({"point2point": 0, "point2plane": 1}[dist] << 8),
            float(nb), float(approximation))


def gen(thr, flags):
    return (wr.GENERIC, float(thr), flags, 0.0)


def case(cid, outliers, k=1, minimizer=2, scene="small", n=None, max_dist=2.0, force_2d=0):
    return dict(id=cid, outliers=outliers, knn=k, minimizer=minimizer, scene=scene, n=n, max_dist=max_dist, force_2d=force_2d)


TRIM = (wr.TRIMMED, 0.85)
CASES = [case(f"median3-k{k}-min{m}", [(wr.MEDIAN, 3.0)], k=k, minimizer=m) for k in (1, 6) for m in (1, 2)]
CASES += [
    case("trimmed0.9+median2.5", [(wr.TRIMMED, 0.9), (wr.MEDIAN, 2.5)]),
    case("maxdist+mindist+trimmed", [(wr.MAXDIST, 0.5), (wr.MINDIST, 0.01), TRIM]),
    case("surfacenormal-k1", [(wr.SURFACENORMAL, 0.9), TRIM]),
    case("surfacenormal-k3", [(wr.SURFACENORMAL, 0.9), TRIM], k=3),
]
for k in (1, 6):
    CASES += [
        case(f"generic-ref-hard-k{k}", [gen(0.5, LARGER), TRIM], k=k),
        case(f"generic-ref-soft-k{k}", [gen(0.0, SOFT), TRIM], k=k),
        case(f"generic-read-hard-k{k}", [gen(0.4, READING), TRIM], k=k),
        case(f"generic-read-soft-k{k}", [gen(0.0, READING | SOFT), TRIM], k=k),
    ]
CASES += [
    case("robust-cauchy-mad", [rob("cauchy", 1.2, "mad")]),
    case("robust-huber-mad-nb3-plane-k1", [rob("huber", 1.2, "mad", nb=3, dist="point2plane")]),
    case("robust-huber-mad-nb3-plane-k6", [rob("huber", 1.2, "mad", nb=3, dist="point2plane")], k=6),
    case("robust-tukey-berg-nb4-apx", [rob("tukey", 0.05, "berg", nb=4, approximation=3.0)]),
    # std runs over EVERY entry of the distance matrix: an unbounded search leaves none infinite
    case("robust-welsch-std-k2+trimmed", [rob("welsch", 1.2, "std"), TRIM], k=2, max_dist=math.inf),
    case("robust-L1-none-p2p", [rob("L1", 1.0, "none")], minimizer=1),
    case("vartrimmed-k1", [(wr.VARTRIMMED, 0.05, 0, 0.99, 0.95)]),
    case("maxdist+vartrimmed-k3-p2p", [(wr.MAXDIST, 1.0), (wr.VARTRIMMED, 0.05, 0, 0.99, 0.95)], k=3, minimizer=1),
    case("trimmed-force2d", [TRIM], force_2d=1),
    case("trimmed-n7", [TRIM], n=7),
    case("trimmed-n300", [TRIM], n=300),
    case("trimmed-n3329", [TRIM], n=3329),
]
# the tail loop behind the prefetched pairs of the pair-sum kernel: more than 2 x 256 x 256 pairs at k = 1, 3 x 1024 x 256 at k > 1
for k in (1, 6):
    CASES += [
        case(f"big-trimmed-k{k}", [TRIM], k=k, scene="big"),
        case(f"big-cauchy-mad-plane-k{k}", [rob("cauchy", 1.2, "mad", dist="point2plane")], k=k, scene="big"),
    ]
IDS = [c["id"] for c in CASES]


def inputs(c):
    """dict(map, normals, reading, read_normals, map_scalar, read_scalar) of a case; the scalars are uniform random rows"""
    sc = weights_scene(c["scene"])
    N = sc["scan"].shape[0]
    n = c["n"] or N
    pick = np.arange(N)[::N // n][:n]   # a short reading is spread over the whole scan
    if n == 7:
        # six pairs survive the trimming and every plane of the scene is axis-aligned: three returns off horizontal faces and two off each
        # kind of wall, picked (best of 300 random draws, the loop replayed on the CPU) so that the 6 x 6 system of the first five iterations
        # keeps a condition number below 4e3 -- a float32 solve of a system at 3e5, what the first / middle / last return of each kind gave, has no margin to SOLVE_TOL
        pick = np.array([62, 2379, 2588, 3470, 4562, 5174, 5599])
        ax = np.abs(sc["scan_normals"][pick]).argmax(1)
        assert sorted(ax.tolist()) == [0, 0, 1, 1, 2, 2, 2]
    rng = np.random.default_rng(11)
    ms = rng.random(sc["map"].shape[0]).astype(np.float32)
    rs = rng.random(N).astype(np.float32)[pick]
    return dict(map=sc["map"], normals=sc["normals"], reading=np.ascontiguousarray(sc["scan"][pick]),
                read_normals=np.ascontiguousarray(sc["scan_normals"][pick]), map_scalar=ms, read_scalar=rs)


def needs(c, what):
    t = [o[0] for o in c["outliers"]]
    if what == "read_normals": return wr.SURFACENORMAL in t
    if what == "map_scalar": return any(o[0] == wr.GENERIC and not (o[2] & READING) for o in c["outliers"])
    if what == "read_scalar": return any(o[0] == wr.GENERIC and (o[2] & READING) for o in c["outliers"])
    raise ValueError(what)


def scale_of(c, j, d2_by_iter):
    """float64 robust scale of iteration j (None: no RobustOutlierFilter in the chain)"""
    for o in c["outliers"]:
        if o[0] == wr.ROBUST:
            return wr.robust_scale(o, j, lambda i: d2_by_iter[i])
    return None


def reference_iteration(c, inp, map_c, p, ids, d2, T_used, j, d2_by_iter, scale_state=None):
    """(chain result, terms, sums, abs) of iteration j over its matches"""
    res = wr.chain_weights(c["outliers"], ids, d2, p, map_c, inp["normals"], inp["read_normals"], T_used, inp["map_scalar"], inp["read_scalar"],
                           iteration=j, d2_of=lambda i: d2_by_iter[i], scale_state=scale_state)
    terms = wr.pair_terms(c["minimizer"], p, map_c, inp["normals"], ids, bool(c["force_2d"]))
    sums, ab = wr.pair_sums(res["w"], terms)
    return res, terms, sums, ab


def cpu_replay(ob, c, iterations=4):
    """the loop on the CPU: the oracle's kd-tree for the matches, this reference for the weights, its float64 step for the pose.  Yields
    (j, chain result, pairs) per iteration."""
    inp = inputs(c)
    mean = inp["map"][:, :3].astype(np.float64).mean(0).astype(np.float32)
    map_c = inp["map"].copy(); map_c[:, :3] = inp["map"][:, :3] - mean[None, :]
    rc = inp["reading"].copy(); rc[:, :3] = inp["reading"][:, :3] - mean[None, :]
    T = np.eye(4, dtype=np.float32)
    d2_by_iter = {}
    for j in range(1, iterations + 1):
        p = ob.transform(T, rc)
        ids, d2 = ob.knn(map_c, p, k=c["knn"], max_dist=c["max_dist"], nthreads=16)
        d2_by_iter[j] = d2
        res, terms, sums, ab = reference_iteration(c, inp, map_c, p, ids, d2, T, j, d2_by_iter)
        yield j, res, int(sums[28])
        T = (wr.step_from_sums(c["minimizer"], sums, bool(c["force_2d"])) @ T.astype(np.float64)).astype(np.float32)
