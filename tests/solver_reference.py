"""float64 numpy reference of the minimisers' algebra, fed with the 32 pair sums a solver worked on (TEST INFRASTRUCTURE: calls
neither the oracle nor the library).

Layout of `sums` (include/icpmi.h: icpmi_minimize_step):
  point to point   [0] sum w, [1:4] sum w p, [4:7] sum w q, [7 + 3 c + r] sum w q_r p_c;
  point to plane   [0:21] upper triangle of A = sum w F F^T row by row, F = [p x n; n], [21:27] b = -sum w F ((p - q) . n),
                   [29:32] force2D's b = -sum w F[2:5] ((p - q)_xy . n_xy);
  both             [27] sum w, [28] pairs.
p is the reading point, q its map point, n the map point's normal, all in the centred frame.

The solvers round the system to float32 before they solve it (H, A, b are float matrices upstream): the reference solves THAT
float32 system in float64, so that what is compared is the solver and not the rounding of its input."""
import numpy as np

EPS_F = float(np.finfo(np.float32).eps)
IU = np.triu_indices(6)


def centre(map4, reading4):
    """setMap's centring: the map's mean in double (sequential sum), differences rounded to float32; the reading moved alike"""
    mean = np.cumsum(map4[:, :3].astype(np.float64), axis=0)[-1] / map4.shape[0]
    mc = map4.copy(); mc[:, :3] = (map4[:, :3].astype(np.float64) - mean).astype(np.float32)
    rc = reading4.copy(); rc[:, :3] = (reading4[:, :3].astype(np.float64) - mean).astype(np.float32)
    return mc, rc, mean


def pair_sums(p, q, n, minimizer, force_2d=False):
    """the 32 sums of the pairs (p_i, q_i, n_i), unit weights, everything in float64"""
    p = np.asarray(p, np.float64)[:, :3]; q = np.asarray(q, np.float64)[:, :3]
    s = np.zeros(32)
    P = p.shape[0]
    s[27], s[28] = P, P
    if minimizer == 1:
        s[0] = P
        s[1:4] = p.sum(0); s[4:7] = q.sum(0)
        S = q.T @ p                                               # S[r, c] = sum q_r p_c
        for c in range(3):
            for r in range(3):
                s[7 + 3 * c + r] = S[r, c]
        return s
    n = np.asarray(n, np.float64)
    Fm = np.concatenate([np.cross(p, n), n], axis=1)
    dot = ((p - q) * n).sum(1)
    s[:21] = (Fm.T @ Fm)[IU]
    s[21:27] = -Fm.T @ dot
    if force_2d:
        dot2 = ((p - q)[:, :2] * n[:, :2]).sum(1)
        s[29:32] = -Fm[:, 2:5].T @ dot2
    return s


def rodrigues(x3):
    th = np.linalg.norm(x3)
    if not th > 0:
        return np.eye(3)
    k = np.asarray(x3, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def h_from_sums(sums):
    """(H float64, H32 = the float32 matrix the solvers decompose, mean_p, mean_q)"""
    w = sums[27]
    mp, mq = sums[1:4] / w, sums[4:7] / w
    S = np.array([[sums[7 + 3 * c + r] for c in range(3)] for r in range(3)])
    H = S - np.outer(mq, sums[1:4])
    return H, H.astype(np.float32), mp, mq


def solve_p2p(sums, is_2d=False):
    """dict: T (4 x 4 float64 optimum), H32, d = det(H32 / |H32|_F), s (singular values), kappa = |H|_F / (s2 + s3) of the polar factor,
    rank, unique, opt = s1 + s2 + sign(det H) s3 (the largest tr(R^T H) over proper rotations)"""
    H, H32, mp, mq = h_from_sums(sums)
    Hd = H32.astype(np.float64)
    nf = np.linalg.norm(Hd)
    T = np.eye(4)
    if is_2d:
        a, b = Hd[0, 0] + Hd[1, 1], Hd[1, 0] - Hd[0, 1]
        r = np.hypot(a, b)
        th = np.arctan2(b, a) if r > 0 else 0.0
        R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
        T[:3, :3] = R; T[:3, 3] = mq - R @ mp
        kappa = (np.linalg.norm(Hd[:2, :2]) / r) if r > 0 else np.inf
        return dict(T=T, H32=H32, d=0.0, s=np.array([r, 0, 0]), kappa=kappa, rank=int(r > 0), unique=bool(r > 0), opt=r, planar=True)
    U, s, Vt = np.linalg.svd(Hd)
    sign = 1.0
    if np.linalg.det(U @ Vt) < 0:
        Vt = Vt.copy(); Vt[-1] *= -1; sign = -1.0
    R = U @ Vt
    T[:3, :3] = R; T[:3, 3] = mq - R @ mp
    d = float(np.linalg.det(Hd / nf)) if nf > 0 else 0.0
    tol = 1e-5 * s[0]
    rank = int((s > tol).sum()) if s[0] > 0 else 0
    unique = rank >= 2 and (sign > 0 or s[1] - s[2] > tol)
    kappa = nf / (s[1] + s[2]) if s[1] + s[2] > 0 else np.inf
    return dict(T=T, H32=H32, d=d, s=s, kappa=kappa, rank=rank, unique=bool(unique), opt=s[0] + s[1] + sign * s[2], planar=False,
                reflect=bool(sign < 0))


def system_from_sums(sums, force_4dof=False, force_2d=False):
    """(A32, b32 as float64 arrays holding float32 values, idx): the N x N system the chain solves and the rows of x it fills"""
    A = np.zeros((6, 6)); A[IU] = sums[:21]; A = A + A.T - np.diag(np.diag(A))
    b = np.array(sums[21:27])
    idx = [0, 1, 2, 3, 4, 5]
    if force_2d:
        idx = [2, 3, 4]; b = b.copy(); b[2:5] = sums[29:32]
    elif force_4dof:
        idx = [2, 3, 4, 5]
    A32 = A.astype(np.float32).astype(np.float64)[np.ix_(idx, idx)]
    b32 = b.astype(np.float32).astype(np.float64)[idx]
    return A32, b32, idx


def chol_pivots(A):
    """the pivots d_j = L_jj^2 of A = L L^T in float64 (NaN after the first non-positive one)"""
    n = A.shape[0]
    L = np.zeros((n, n)); piv = np.full(n, np.nan)
    for j in range(n):
        d = A[j, j] - (L[j, :j] ** 2).sum()
        piv[j] = d
        if not d > 0:
            break
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return piv


def solve_p2l(sums, force_4dof=False, force_2d=False, keep_factor=1.0):
    """dict: T, x (6,), A32, b32, idx, lam (eigenvalues ascending), Q, thr = N eps_f lam_max (the rule's threshold), kept (lam > keep_factor
    thr), kappa = lam_max / smallest kept, piv (float64 Cholesky pivots), pthr = N eps_f max A_jj"""
    A32, b32, idx = system_from_sums(sums, force_4dof, force_2d)
    N = len(idx)
    lam, Q = np.linalg.eigh(A32)
    lmax = float(np.abs(lam).max())
    thr = N * EPS_F * lmax
    kept = lam > keep_factor * thr
    xs = np.zeros(N)
    for e in np.nonzero(kept)[0]:
        xs += Q[:, e] * (Q[:, e] @ b32) / lam[e]
    x = np.zeros(6); x[idx] = xs
    T = np.eye(4); T[:3, :3] = rodrigues(x[:3]); T[:3, 3] = x[3:]
    kappa = lmax / lam[kept].min() if kept.any() else np.inf
    return dict(T=T, x=x, A32=A32, b32=b32, idx=idx, lam=lam, Q=Q, thr=thr, kept=kept, kappa=kappa, piv=chol_pivots(A32),
                pthr=N * EPS_F * float(np.diag(A32).max()))


def x_from_T(T):
    """(rotation vector, translation) of a point-to-plane step"""
    R = np.asarray(T, np.float64)[:3, :3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(v), (np.trace(R) - 1.0) / 2.0
    th = np.arctan2(s, c)
    rv = v * (th / s) if s > 0 else np.zeros(3)
    return np.concatenate([rv, np.asarray(T, np.float64)[:3, 3]])


def pose_error(Ta, Tb):
    Ta = np.asarray(Ta, np.float64); Tb = np.asarray(Tb, np.float64)
    dt = float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3]))
    R = Ta[:3, :3].T @ Tb[:3, :3]
    c = (np.trace(R) - 1.0) / 2.0
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return dt, float(np.arctan2(s, c))


# ---------------------------------------------------------------------------------------------------------------- the checks
def branch_margin(case, ref):
    """(ok, text): is the case inside the branch it is meant for, by the margins of its kind -- established from the data"""
    route = case["route"]
    if route in ("svd", "newton"):
        d = ref["d"]
        return (d < 1e-7) if route == "svd" else (d > 1e-5), f"d = {d:.3e}"
    if route == "reflect":                  # the reflection repair runs: d a decade below -1e-6 and det(U V^T) < 0 in the float64 SVD
        return ref["d"] < -1e-5 and ref["reflect"], f"d = {ref['d']:.3e}, det(U V^T) {'<' if ref['reflect'] else '>'} 0"
    if route == "zero":                     # A == 0 exactly: threshold 0, nothing kept
        return not ref["A32"].any() and not ref["kept"].any(), f"max |A| = {np.abs(ref['A32']).max():.1e}"
    if route == "planar":
        return True, f"r = {ref['s'][0]:.3e}"
    if route == "either":
        return True, (f"d = {ref['d']:.3e}" if "d" in ref else
                      f"lam / thr = {np.array2string(ref['lam'] / ref['thr'], precision=2)}, min pivot / pthr = {np.nanmin(ref['piv']) / ref['pthr']:.1e}")
    piv_min = np.nanmin(ref["piv"])
    if route == "chol":
        return bool(np.all(ref["piv"] > 1e3 * ref["pthr"])), f"min pivot / (N eps max A_jj) = {piv_min / ref['pthr']:.3e}"
    big = ref["lam"] > 1e3 * ref["thr"]
    zero = np.abs(ref["lam"]) < 1e-3 * ref["thr"]
    n_null = len([i for i in case["null"] if i in ref["idx"]])
    ok = bool(np.all(big | zero)) and int(zero.sum()) == n_null and n_null > 0 and not piv_min > ref["pthr"]
    lz = np.abs(ref["lam"][zero]).max() / ref["thr"] if zero.any() else np.nan
    lb = ref["lam"][big].min() / ref["thr"] if big.any() else np.nan
    return ok, f"zero lam / thr <= {lz:.1e}, others >= {lb:.1e}, min pivot / pthr = {piv_min / ref['pthr']:.1e}"


def check_step(case, T, sums, mc, rc, consts, what, sums_exact=True):
    """Assertions 1 - 4 of one single step (T 4 x 4, sums[32]) over the centred pairs (rc_i, mc_i); returns the figures.
    consts: the module solver_cases (bounds)."""
    kw = case["kw"]
    mini = kw["minimizer"]
    f2d, f4, is2d = bool(kw.get("force_2d")), bool(kw.get("force_4dof")), bool(kw.get("is_2d"))
    name = case["name"]
    T = np.asarray(T, np.float64)
    sums = np.asarray(sums, np.float64)
    fig = dict(name=name)
    # ---- 1: the sums
    want = pair_sums(rc, mc, case["normals"], mini, f2d)
    assert sums[28] == case["pairs"] and sums[27] == case["pairs"], (what, name, sums[27], sums[28])
    if mini == 1:
        scale = max(np.abs(want[7:16]).max(), 1e-30) / consts.GOLDEN_AJJ
        np.testing.assert_allclose(sums[:16], want[:16], rtol=consts.SUM_RTOL_A, atol=consts.SUM_ATOL * scale, err_msg=f"{what} {name} sums")
        assert np.all(sums[16:27] == 0.0) and np.all(sums[29:32] == 0.0), (what, name)
    else:
        A = np.zeros((6, 6)); A[IU] = want[:21]
        scale = np.diag(A).max() / consts.GOLDEN_AJJ
        np.testing.assert_allclose(sums[:21], want[:21], rtol=consts.SUM_RTOL_A, atol=consts.SUM_ATOL * scale, err_msg=f"{what} {name} A")
        np.testing.assert_allclose(sums[21:27], want[21:27], rtol=consts.SUM_RTOL_B, atol=consts.SUM_ATOL * scale, err_msg=f"{what} {name} b")
        if f2d:
            np.testing.assert_allclose(sums[29:32], want[29:32], rtol=consts.SUM_RTOL_B, atol=consts.SUM_ATOL * scale, err_msg=f"{what} {name} b2d")
        else:
            assert np.all(sums[29:32] == 0.0), (what, name)
        Ad = np.zeros((6, 6)); Ad[IU] = sums[:21]; Ad = Ad + Ad.T
        for i in case["null"]:
            if i in ((2, 3, 4) if f2d else ((2, 3, 4, 5) if f4 else range(6))):
                # zero by construction: the row of A, b's entry (and force2D's)
                assert np.all(Ad[i] == 0.0) and sums[21 + i] == 0.0, (what, name, i, Ad[i], sums[21 + i])
                if f2d:
                    assert sums[29 + i - 2] == 0.0, (what, name, i)
    # ---- 3: universal properties
    assert np.isfinite(T).all(), (what, name, T)
    assert np.array_equal(T[3], [0, 0, 0, 1]), (what, name, T[3])
    R = T[:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-5 and abs(np.linalg.det(R) - 1.0) <= 1e-5, (what, name, R)
    if mini == 1:
        ref = solve_p2p(sums, is2d)
        Hd = ref["H32"].astype(np.float64)
        got = float(np.trace(R.T @ Hd))
        fig["opt_gap"] = ref["opt"] - got
        assert got >= ref["opt"] * (1 - 1e-5) - 1e-6 * np.linalg.norm(Hd), (what, name, got, ref["opt"])
        if case["pairing"] == "distance":      # all points coincide: H == 0, the documented identity rotation, t = mean_q - mean_p
            assert not ref["H32"].any(), (what, name, ref["H32"])
            assert np.array_equal(R, np.eye(3)), (what, name, R)
            assert np.array_equal(T[:3, 3].astype(np.float32), (mc[0, :3].astype(np.float64) - rc[0, :3]).astype(np.float32)), (what, name, T[:3, 3])
        if is2d:
            assert T[2, 3] == 0 and np.array_equal(R[2], [0, 0, 1]) and np.array_equal(R[:, 2], [0, 0, 1]), (what, name, T)
    else:
        ref = solve_p2l(sums, f4, f2d)
        x = x_from_T(T)
        fig["x"] = x
        idx = ref["idx"]
        obs = ref["lam"] > (1e3 * ref["thr"] if case["route"] == "either" else ref["thr"])
        Qo = ref["Q"][:, obs]
        res = Qo.T @ (ref["A32"] @ x[idx] - ref["b32"])
        fig["residual"] = float(np.linalg.norm(res) / max(np.linalg.norm(ref["b32"]), 1e-300))
        assert np.linalg.norm(res) <= 1e-4 * np.linalg.norm(ref["b32"]), (what, name, fig["residual"])
        for i in range(6):
            if i not in idx or i in case["null"]:
                assert x[i] == 0.0, (what, name, "x", i, x)           # exactly: never written, or axis-aligned null space
        if case["route"] == "minnorm":
            Qn = ref["Q"][:, ~ref["kept"]]
            assert np.abs(Qn.T @ x[idx]).max() <= 1e-6 * max(np.linalg.norm(x), 1e-30), (what, name)
        if case["route"] == "either":
            # which route ran, from the data: a float64 pivot a decade below the rule's threshold cannot pass the float32 test (its rounding
            # is a few eps_f A_jj, the threshold N eps_f max A_jj), so the minimum-norm route ran and x has nothing along the dropped
            # eigenvectors; Cholesky through such a pivot would leave (q . b) / pivot there
            Qn = ref["Q"][:, ref["lam"] <= 1e3 * ref["thr"]]
            fig["null_part"] = float(np.abs(Qn.T @ x[idx]).max()) if Qn.size else 0.0
            if not np.nanmin(ref["piv"]) > 0.1 * ref["pthr"]:
                assert fig["null_part"] <= 1e-6, (what, name, "not the minimum-norm solution", fig["null_part"])
    # ---- 2: branch membership (a case outside its margin is a broken fixture)
    ok, text = branch_margin(case, ref)
    fig["margin"] = text
    assert ok, (what, name, "not inside its branch", text)
    # ---- 4: value
    kappa = ref["kappa"]
    fig["kappa"] = kappa
    if mini == 2 and case["route"] == "either":
        xr = ref["x"]
        big = ref["lam"] > 1e3 * ref["thr"]
        Qb = ref["Q"][:, big]
        kb = float(ref["lam"].max() / ref["lam"][big].min())
        err = float(np.linalg.norm(Qb.T @ (x[idx] - xr[idx])))
        fig["kappa"] = kb
        fig["ratio"] = err / (EPS_F * kb)
        fig["bound"] = max(consts.DR_FLOOR, consts.K * EPS_F * kb)
        fig["err"] = (err, err)
        assert err <= fig["bound"], (what, name, err, fig["bound"])
    elif case["unique"]:
        assert ref.get("unique", True), (what, name, "fixture: the optimum is not unique")
        dt, dr = pose_error(T, ref["T"])
        fig["err"] = (dt, dr)
        fig["ratio"] = max(dr, dt) / (EPS_F * kappa)
        bt = max(consts.DT_FLOOR, consts.K * EPS_F * kappa)
        br = max(consts.DR_FLOOR, consts.K * EPS_F * kappa)
        fig["bound"] = (bt, br)
        assert dt <= bt and dr <= br, (what, name, (dt, dr), (bt, br), kappa)
    fig["ref"] = ref
    return fig


def line(fig):
    e = fig.get("err")
    return (f"{fig['name']:28s} {fig['margin']:72s} kappa {fig['kappa']:9.3e}"
            + (f"  dt {e[0]:.2e} dr {e[1]:.2e}  err / (eps kappa) {fig['ratio']:.3f}" if e else "  (optimum not unique: properties only)"))
