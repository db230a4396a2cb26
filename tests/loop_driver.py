"""What the loop tests share (test_gpu_loop_matches.py, test_gpu_loop_weights.py): the float32 pose conversions of the library's host side
restated through the oracle's transform, and the scenes, built once per process."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32T(T):
    return np.asarray(T, dtype=np.float32)


def mat4_mul_f32(ob, A, B):
    """A @ B as the library's host_mat4_mul forms it: column j of the product is column j of B moved by A through the transform's fmaf
    chain (rows 0-2); row 3 of a product of rigid transforms is row 3 of B"""
    out = ob.transform(f32T(A), np.ascontiguousarray(f32T(B).T))
    R = np.array(out.T, dtype=np.float32)
    R[3] = f32T(B)[3]
    return R


def pose_out(ob, T_c, mean):
    """the caller-frame pose the library returns for the centred-frame T_c: [I | mean] T_c [I | -mean]"""
    Tm = np.eye(4, dtype=np.float32); Tm[:3, 3] = mean
    Tmi = np.eye(4, dtype=np.float32); Tmi[:3, 3] = -mean
    return mat4_mul_f32(ob, Tm, mat4_mul_f32(ob, T_c, Tmi))


def centring(mean):
    T = np.eye(4, dtype=np.float32); T[:3, 3] = -mean
    return T


# ------------------------------------------------------------------------------------------------------------------ scenes
_scenes = {}
DENSE_SPOT_MAP, DENSE_SPOT_READING = 2000, 256   # the sizes of scene "dense_spot" (test_piece_list_overflow states what they guarantee)


def ball(rng, count, radius):
    """count points uniform in the ball of that radius around the origin, float64"""
    v = rng.normal(size=(count, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v * (radius * rng.uniform(0.0, 1.0, (count, 1)) ** (1.0 / 3.0))


def scene(name):
    """(map (M,4) f32, map normals (M,3) f32 or None, reading (N,4) f32); built once per module"""
    if name in _scenes:
        return _scenes[name]
    from norlab_icp_mapper_amd import synth
    if name in ("mid", "far", "misaligned", "exact_hits", "clusters", "dense_spot"):
        sc = _scenes.get("_mid_raw") or synth.make_scene(m=200_000, n=20_000)
        _scenes["_mid_raw"] = sc
        mp, nm, rd = sc["map"], sc["normals"], sc["scan"]
        rng = np.random.default_rng(29)
        if name == "far":       # 2 000 returns 100 - 250 m outside the map: unbounded maxDist sends them through the brute pass
            far = np.ones((2000, 4), np.float32)
            far[:, :3] = rng.uniform(-1, 1, (2000, 3)) * np.array([50.0, 50.0, 5.0]) + np.array([200.0, -150.0, 5.0])
            rd = np.r_[rd, far]
        elif name == "misaligned":  # ~0.15 rad / 1.5 m on top of the scene's own offset: the first seeds land far from the answer
            Tx = synth.make_T((0.08, -0.05, 0.12), (1.2, -0.8, 0.5)).astype(np.float32)
            import oracle_bindings as ob
            rd = ob.transform(Tx, rd)
        elif name == "exact_hits":  # map points inside the reading: exact zeros in the first iteration's d2
            rd = np.r_[rd, mp[rng.choice(mp.shape[0], 1500, replace=False)]]
        elif name == "clusters":    # 60 spots under the reading holding 30 copies of one map point each: list overflow + index ties
            near = rng.choice(mp.shape[0], 60, replace=False)
            mp = np.r_[mp, np.repeat(mp[near], 30, axis=0)]
            nm = np.r_[nm, np.repeat(nm[near], 30, axis=0)]
        elif name == "dense_spot":  # 2 000 distinct map points and 256 reading points inside one 2 cm ball each: the piece list overflows
            i0 = int(rng.integers(0, rd.shape[0]))
            spot = (sc["T_gt"] @ rd[i0].astype(np.float64))[:3]           # where reading point i0 lies in the map frame
            extra = np.ones((DENSE_SPOT_MAP, 4), np.float32)
            extra[:, :3] = spot + ball(rng, DENSE_SPOT_MAP, 0.02)
            assert np.unique(extra[:, :3], axis=0).shape[0] == DENSE_SPOT_MAP    # distinct positions: nnk_wg_kernel's CAPQ passes shrink
            nearest = np.argmin(((mp[:, :3].astype(np.float64) - spot) ** 2).sum(1))
            mp = np.r_[mp, extra]
            nm = np.r_[nm, np.repeat(nm[nearest][None, :], DENSE_SPOT_MAP, axis=0)]
            more = np.ones((DENSE_SPOT_READING, 4), np.float32)
            more[:, :3] = rd[i0, :3].astype(np.float64) + ball(rng, DENSE_SPOT_READING, 0.02)
            rd = np.r_[rd, more]
        out = (np.ascontiguousarray(mp), np.ascontiguousarray(nm), np.ascontiguousarray(rd))
    elif name == "bundled":  # map = bundled scans 0-3 placed by the trajectory, reading = scan 4 placed the same way
        import oracle_bindings as ob
        from config4_data import quat_T
        z = np.load(os.path.join(ROOT, "tests", "golden", "bundled_scans_all.npz"))
        def placed(i):
            p = np.ones((z[f"scan{i}_xyz"].shape[0], 4), np.float32); p[:, :3] = z[f"scan{i}_xyz"]
            return ob.transform(quat_T(z["trajectory"][i][2:]), p)
        mp = np.concatenate([placed(i) for i in range(4)])
        out = (mp, None, placed(4))
    elif name == "headline":
        sc = synth.make_scene(m=1_000_000, n=100_000)
        out = (sc["map"], sc["normals"], sc["scan"])
    else:
        raise ValueError(name)
    _scenes[name] = out
    return out


def weights_scene(name):
    """dict(map, normals, scan, scan_normals) of the loop-weights tests, the misalignment of `mid`: "small" = 60 000 x 6 000 points, "big" =
    200 000 x 135 000 (the scan generator drawn further: 135 000 independent returns, none twice); built once per process"""
    key = "_w_" + name
    if key not in _scenes:
        from norlab_icp_mapper_amd import synth
        m, n = {"small": (60_000, 6_000), "big": (200_000, 135_000)}[name]
        _scenes[key] = synth.make_scene(m=m, n=n)
    return _scenes[key]
