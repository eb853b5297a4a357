"""Scenes and restatements for msorb_create_new_map_points_kf (the neighbour loop of LocalMapping::CreateNewMapPoints,
src/LocalMapping.cc:460-731; line numbers below are that file's unless another is named).

make_scene     one current KeyFrame and K neighbours on a forward-plus-sideways trajectory over shared 3-D points
degenerate     hand-built pairs for the `continue`s that no consistent scene reaches
R32            the loop in float32 numpy, the fixed steps of ms-slam_amd/csrc/new_points_device.h, vectorised over the pairs of a neighbour
R64            the same with numpy.linalg.svd in float64 on the float A, libm's cos(2 atan2()) and float64 arithmetic
stale          R32 with the masks of the current KeyFrame never updated: what one batched search over all neighbours computes
"""
import numpy as np

import bow_cases
import bow_match_cases as bmc

(NONE, TRIANGULATED, STEREO1, STEREO2, LOW_PARALLAX, NULL_W, STEREO_DEPTH, BEHIND1, BEHIND2, REPROJ1, REPROJ2, ZERO_DIST, FAR,
 SCALE_RATIO) = range(14)
STATUS_NAMES = ("none", "triangulated", "stereo1", "stereo2", "low_parallax", "null_w", "stereo_depth", "behind1", "behind2",
                "reproj1", "reproj2", "zero_dist", "far", "scale_ratio")
N_LEVELS = 8
SCALE = (np.float32(1.2) ** np.arange(N_LEVELS)).astype(np.float32)
SIGMA2 = (SCALE * SCALE).astype(np.float32)
CAM = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, mb=0.5371657, mbf=386.1448)
MAX_SWEEPS = 60   # kNpMaxSweeps


def _rot(a):
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))


def geometry(R, t, cam, u_right, depth):
    """the geometry block of one KeyFrame: what GetPose / GetCameraCenter / the camera members hold, as float32"""
    f = np.float32
    g = dict(Tcw=np.concatenate([R, t[:, None]], 1).astype(f), Ow=(-R.T @ t).astype(f), u_right=np.asarray(u_right, f),
             depth=np.asarray(depth, f))
    for k in ("fx", "fy", "cx", "cy", "mb", "mbf"):
        g[k] = f(cam[k])
    g["invfx"], g["invfy"] = f(1) / g["fx"], f(1) / g["fy"]
    return g


def epipolar(R1, t1, R2, t2, cam1, cam2):
    """F12 and ep as msorb_triangulation_kf_pair wants them (float64 here, narrowed once)"""
    R12, t12 = R1 @ R2.T, t1 - R1 @ R2.T @ t2
    K1 = np.array([[cam1["fx"], 0, cam1["cx"]], [0, cam1["fy"], cam1["cy"]], [0, 0, 1.0]])
    K2 = np.array([[cam2["fx"], 0, cam2["cx"]], [0, cam2["fy"], cam2["cy"]], [0, 0, 1.0]])
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = (np.linalg.inv(K1.T) @ tx @ R12 @ np.linalg.inv(K2)).astype(np.float32)
    C = R2 @ (-R1.T @ t1) + t2
    z = C[2] if abs(C[2]) > 1e-9 else 1e-9
    ep = np.array([cam2["fx"] * C[0] / z + cam2["cx"], cam2["fy"] * C[1] / z + cam2["cy"]], np.float32)
    return F12, ep


def make_scene(seed, n1=300, K=3, n2=None, n_nodes=12, stereo_frac=0.4, pix_noise=0.6, dup_frac=0.12, far_frac=0.08,
               mask_frac=0.15, octave_jitter=0.15, wild_angle=0.15, th_far=0.0, inertial=False, coarse=False,
               check_orientation=True, disjoint_nodes=(), flip=12, depth_hi=40.0, step=(1.5, 0.05, 1.0)):
    """-> dict(kfs [K + 1] (kps, desc, fv, geometry), valid1, avail2 [K], F12 [K], ep [K], coarse, check_orientation, inertial,
    th_far).  KeyFrame 0 is the current one.  Feature i of a KeyFrame observes point pt[i] with pixel noise; some features of
    KeyFrame 0 observe the same point twice (dup_frac), so that a later query of a node wants the train an earlier one claims;
    far_frac of the points are too far for parallax; octave_jitter of the octaves disagree with the distance; neighbours in
    disjoint_nodes share no BoW node with KeyFrame 0."""
    rng = np.random.default_rng(seed)
    n2 = [n1 + 17 * (k + 1) for k in range(K)] if n2 is None else ([n2] * K if np.isscalar(n2) else list(n2))
    ns = [n1] + n2
    P = max(max(ns), 1)
    fx, fy, cx, cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]
    z = rng.uniform(4, depth_hi, P)
    far = rng.random(P) < far_frac
    z[far] = rng.uniform(400, 600, int(far.sum()))
    Xw = np.stack([(rng.uniform(0, 1241, P) - cx) / fx * z, (rng.uniform(0, 376, P) - cy) / fy * z, z], 1)
    base_desc = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    node_of_point = rng.integers(0, n_nodes, P) * 5 + 2
    base_angle = rng.uniform(0, 360, P)
    kfs, poses = [], []
    for k, n in enumerate(ns):
        R = _rot(rng.normal(0, 0.02, 3))
        C = np.array(step) * k * (1 if k % 2 else -1) * np.array([1, 1, -1 if k % 2 == 0 else 1]) + rng.normal(0, 0.03, 3) * (k > 0)
        if k:
            C[2] = step[2] * k   # forward
        t = -R @ C
        if k == 0:
            n_dup = int(dup_frac * n)
            pt = np.concatenate([rng.permutation(P)[:n - n_dup], np.zeros(n_dup, np.int64)])
            if n_dup:
                pt[n - n_dup:] = rng.choice(pt[:n - n_dup], n_dup)
            pt = pt[rng.permutation(n)] if n else pt
        else:
            pt = rng.permutation(P)[:n] if n <= P else rng.integers(0, P, n)
        Xc = Xw[pt] @ R.T + t
        zc = np.where(np.abs(Xc[:, 2]) < 0.3, 0.3, Xc[:, 2])
        u = fx * Xc[:, 0] / zc + cx + rng.normal(0, pix_noise, n)
        v = fy * Xc[:, 1] / zc + cy + rng.normal(0, pix_noise, n)
        kps = np.zeros(n, bmc.KP_DTYPE)
        kps["x"], kps["y"] = u, v
        dist = np.linalg.norm(Xc, axis=1)
        octv = np.clip(np.round(np.log(np.maximum(dist, 1e-3) / 6.0) / np.log(1.2)), 0, N_LEVELS - 1).astype(np.int64)
        jit = rng.random(n) < octave_jitter
        octv[jit] = rng.integers(0, N_LEVELS, int(jit.sum()))
        kps["octave"] = octv
        ang = np.mod(base_angle[pt] + 9.0 * k + rng.normal(0, 4, n), 360)
        wild = rng.random(n) < wild_angle
        ang[wild] = rng.uniform(0, 360, int(wild.sum()))
        kps["angle"] = ang
        stereo = (rng.random(n) < stereo_frac) & (zc > 0.5) & ~far[pt]   # (no disparity to speak of at 400 m)
        ur = np.where(stereo, u - CAM["mbf"] / zc + rng.normal(0, 0.3, n), -1.0).astype(np.float32)
        stereo &= (kps["x"] - ur) > 0.05
        ur = np.where(stereo, ur, np.float32(-1))
        with np.errstate(divide="ignore", invalid="ignore"):
            depth = np.where(stereo, np.float32(CAM["mbf"]) / (kps["x"] - ur), np.float32(-1)).astype(np.float32)
        desc = bow_cases._flip_bits(rng, base_desc[pt], rng.integers(0, flip + 1, n)) if n else np.zeros((0, 32), np.uint8)
        node = node_of_point[pt] + (1 if k in disjoint_nodes else 0)
        kfs.append(dict(kps=kps, desc=np.ascontiguousarray(desc), fv=bmc.feature_vector_from_nodes(node),
                        geometry=geometry(R, t, CAM, ur, depth), pt=pt))
        poses.append((R, t))
    sc = dict(kfs=kfs, valid1=(rng.random(n1) >= mask_frac).astype(np.uint8),
              avail2=[(rng.random(n) >= mask_frac).astype(np.uint8) for n in n2], F12=[], ep=[], coarse=coarse,
              check_orientation=check_orientation, inertial=inertial, th_far=float(th_far))
    for k in range(1, K + 1):
        F12, ep = epipolar(*poses[0], *poses[k], CAM, CAM)
        sc["F12"].append(F12)
        sc["ep"].append(ep)
    return sc


def degenerate():
    """Seven hand-built pairs, one per neighbour, each the only feature of its neighbour and in reach of one feature of the current
    KeyFrame (same descriptor, one BoW node, coarse search, no orientation filter): the `continue`s of :607 (x3Dh(3) == 0), :630
    (stereo depth <= 0), :635, :639, :654, :691 and :702.  Intrinsics with exactly representable quotients; the current KeyFrame at
    the origin.  Two neighbours need inputs no consistent KeyFrame has: a Tcw whose second and third rotation rows are parallel (rows
    and column 3 of A then decouple and the smallest singular vector has w == 0 exactly), and a camera centre that is the
    triangulated point itself (set after a first run of R32)."""
    f = np.float32
    cam = dict(fx=512.0, fy=512.0, cx=320.0, cy=256.0, mb=0.5, mbf=256.0)
    rng = np.random.default_rng(99)
    I3 = np.eye(3)

    def px(a, b):
        return cam["fx"] * a + cam["cx"], cam["fy"] * b + cam["cy"]

    # (a1, b1, ur1, depth1), the neighbour's (R, t), (a2, b2, ur2, depth2)
    rows = [
        ((0.25, 0.0, -1, -1), (I3, np.zeros(3)), (-0.25, 0.5, -1, -1)),            # NULL_W: its Tcw is overwritten below
        ((0.0, 0.0, 300.0, 0.0), (I3, np.array([-1.0, 0, 0])), (-0.1, 0.0, -1, -1)),  # STEREO_DEPTH: stereo with depth 0
        ((-0.25, 0.0, -1, -1), (I3, np.array([-1.0, 0, 0])), (0.25, 0.0, -1, -1)),  # BEHIND1: the rays meet behind both cameras
        ((0.0, 0.0, -1, -1), (I3, np.array([-1.0, 0, -10.0])), (0.2, 0.0, -1, -1)),  # BEHIND2: (0, 0, 5) seen from (1, 0, 10)
        ((0.125, 0.0, -1, -1), (I3, np.array([-1.0, 0, 0])), (-0.125, 0.0625, -1, -1)),  # REPROJ1: skew rays, 32 px apart in v
        ((0.125, 0.0, -1, -1), (I3, np.array([-1.0, 0, 0])), (-0.125, 0.0, 100.0, 4.0)),  # REPROJ2: u_right far from u - mbf / z
        ((0.125, 0.125, -1, -1), (I3, np.array([-1.0, 0, 0])), (-0.125, 0.125, -1, -1)),  # ZERO_DIST: Ow2 := x3D below
    ]
    K = len(rows)
    desc = rng.integers(0, 256, (K, 32), dtype=np.uint8)
    kps1 = np.zeros(K, bmc.KP_DTYPE)
    ur1, d1 = np.zeros(K, f), np.zeros(K, f)
    kfs = [None]
    sc = dict(valid1=np.ones(K, np.uint8), avail2=[], F12=[], ep=[], coarse=True, check_orientation=False, inertial=False, th_far=0.0)
    for k, (q1, (R, t), q2) in enumerate(rows):
        kps1["x"][k], kps1["y"][k] = px(q1[0], q1[1])
        ur1[k], d1[k] = q1[2], q1[3]
        kp2 = np.zeros(1, bmc.KP_DTYPE)
        kp2["x"][0], kp2["y"][0] = px(q2[0], q2[1])
        g = geometry(R, t, cam, [q2[2]], [q2[3]])
        kfs.append(dict(kps=kp2, desc=desc[k:k + 1].copy(), fv=bmc.feature_vector_from_nodes([7]), geometry=g))
        sc["avail2"].append(np.ones(1, np.uint8))
        sc["F12"].append(np.zeros((3, 3), f))              # coarse: not read
        sc["ep"].append(np.array([1e6, 1e6], f))           # far from every keypoint
    kfs[0] = dict(kps=kps1, desc=desc, fv=bmc.feature_vector_from_nodes([7] * K), geometry=geometry(I3, np.zeros(3), cam, ur1, d1))
    kfs[1]["geometry"]["Tcw"] = np.array([[1, 0, 0, 0], [0, 0, 0.5, 5], [0, 0, 1, 0]], f)   # row 1 = b2 * row 2, b2 = 0.5
    sc["kfs"] = kfs
    first = R32(sc)
    assert first[6]["status"][6] == TRIANGULATED
    kfs[7]["geometry"]["Ow"] = first[6]["x3D"][6].copy()
    return sc


SCENES = {
    "plain": lambda: make_scene(1, n1=257, K=3),
    "reclaimed": lambda: make_scene(1, n1=257, K=3, dup_frac=0.3, mask_frac=0.05),
    "inertial_far": lambda: make_scene(2, n1=200, K=2, inertial=True, th_far=30.0, far_frac=0.15),
    "coarse_noorient": lambda: make_scene(1, n1=200, K=2, coarse=True, check_orientation=False, pix_noise=2.5),
    "degenerate": degenerate,
}


# ---------------------------------------------------------------------------------------------------------------------
# the per-pair arithmetic (ms-slam_amd/csrc/new_points_device.h)
# ---------------------------------------------------------------------------------------------------------------------
def jacobi_null_vector32(A):
    """np_null_vector over A [m, 4, 4] float32: the restated Eigen::JacobiSVD<Matrix4f>, every lane with its own sweep count"""
    f = np.float32
    A = np.asarray(A, f)
    m = len(A)
    tiny, precision = f(1.17549435e-38), f(2.384185791015625e-07)

    def mx(a, b):
        return np.where(b > a, b, a)

    scale = np.zeros(m, f)
    for e in np.abs(A).reshape(m, 16).T:
        scale = mx(scale, e)
    scale = np.where(scale == 0, f(1), scale)
    W = (A / scale[:, None, None]).astype(f)
    V = np.tile(np.eye(4, dtype=f), (m, 1, 1))
    aW = np.abs(W)
    max_diag = mx(mx(aW[:, 0, 0], aW[:, 1, 1]), mx(aW[:, 2, 2], aW[:, 3, 3]))
    done = np.zeros(m, bool)
    with np.errstate(all="ignore"):
        for _ in range(MAX_SWEEPS):
            rotated = np.zeros(m, bool)
            for p in range(1, 4):
                for q in range(p):
                    thr = mx(np.full(m, tiny), precision * max_diag)
                    act = ~done & ((np.abs(W[:, p, q]) > thr) | (np.abs(W[:, q, p]) > thr))
                    if not act.any():
                        continue
                    rotated |= act
                    m00, m01, m10, m11 = W[:, p, p], W[:, p, q], W[:, q, p], W[:, q, q]
                    t, d = m00 + m11, m10 - m01
                    nz = ~(np.abs(d) < tiny)
                    u = t / d
                    tmp = np.sqrt(f(1) + u * u)
                    s1 = np.where(nz, f(1) / tmp, f(0))
                    c1 = np.where(nz, u / tmp, f(1))
                    n00, n01, n11 = c1 * m00 + s1 * m10, c1 * m01 + s1 * m11, c1 * m11 - s1 * m01
                    deno = f(2) * np.abs(n01)
                    nzr = ~(deno < tiny)
                    tau = (n00 - n11) / deno
                    w = np.sqrt(tau * tau + f(1))
                    tt = np.where(tau > 0, f(1) / (tau + w), f(1) / (tau - w))
                    n = f(1) / np.sqrt(tt * tt + f(1))
                    mag = np.abs(tt) * n
                    sr = np.where(nzr, np.where((tt > 0) == (n01 > 0), -mag, mag), f(0))
                    cr = np.where(nzr, n, f(1))
                    cl, sl = c1 * cr + s1 * sr, s1 * cr - c1 * sr
                    Wn = W.copy()
                    a, b = W[:, p, :], W[:, q, :]
                    Wn[:, p, :] = cl[:, None] * a + sl[:, None] * b
                    Wn[:, q, :] = cl[:, None] * b - sl[:, None] * a
                    a, b = Wn[:, :, p].copy(), Wn[:, :, q].copy()
                    Wn[:, :, p] = cr[:, None] * a - sr[:, None] * b
                    Wn[:, :, q] = sr[:, None] * a + cr[:, None] * b
                    Vn = V.copy()
                    a, b = V[:, :, p], V[:, :, q]
                    Vn[:, :, p] = cr[:, None] * a - sr[:, None] * b
                    Vn[:, :, q] = sr[:, None] * a + cr[:, None] * b
                    W = np.where(act[:, None, None], Wn, W)
                    V = np.where(act[:, None, None], Vn, V)
                    max_diag = np.where(act, mx(max_diag, mx(np.abs(W[:, p, p]), np.abs(W[:, q, q]))), max_diag)
            done |= ~rotated
            if done.all():
                break
    x = np.zeros((m, 4), f)
    for i in range(m):   # descending order by selection with swaps: first maximum of the tail, stop at a zero maximum
        sv = [abs(W[i, j, j]) for j in range(4)]
        col = [0, 1, 2, 3]
        for j in range(4):
            pos = j
            for k in range(j + 1, 4):
                if sv[k] > sv[pos]:
                    pos = k
            if sv[pos] == 0:
                break
            if pos != j:
                sv[j], sv[pos] = sv[pos], sv[j]
                col[j], col[pos] = col[pos], col[j]
        x[i] = V[i, :, col[3]]
    return x


def cos_stereo32(mb, depth):
    """np_cos_stereo: (d^2 - h^2) / (d^2 + h^2) in double from the float inputs, h = mb / 2 as a float"""
    h, d = (np.float32(mb) / np.float32(2)).astype(np.float64), np.asarray(depth, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return ((d * d - h * h) / (d * d + h * h)).astype(np.float32)


def cos_stereo_libm32(mb, depth):
    """cos(2 * atan2(mb / 2, depth)) with numpy's float32 functions (:591)"""
    f = np.float32
    return np.cos(f(2) * np.arctan2(np.full(np.shape(depth), f(mb) / f(2), f), np.asarray(depth, f)))


def pair_math(g1, g2, f1, f2, inertial, th_far, ratio_factor, F):
    """:578-712 over m pairs.  g: geometry dicts; f: dict(u, v, ur, depth, sigma2, scale) of float32 [m]; F = numpy.float32 (the
    header's steps) or numpy.float64 (R64).  -> status uint8 [m], x3D F [m, 3], comparisons {name: (lhs, rhs, scale, reached)}"""
    exact = F is np.float32
    m = len(f1["u"])
    T1, T2 = np.asarray(g1["Tcw"], np.float32).astype(F), np.asarray(g2["Tcw"], np.float32).astype(F)
    O1, O2 = np.asarray(g1["Ow"], np.float32).astype(F), np.asarray(g2["Ow"], np.float32).astype(F)
    c1 = {k: F(g1[k]) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")}
    c2 = {k: F(g2[k]) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")}
    q1 = {k: np.asarray(v, np.float32).astype(F) for k, v in f1.items()}
    q2 = {k: np.asarray(v, np.float32).astype(F) for k, v in f2.items()}
    one = F(1)
    comps = {}

    def dot3(a, b):   # a, b: triples of arrays / scalars; (a0 b0 + a1 b1) + a2 b2
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    with np.errstate(all="ignore"):
        st1, st2 = q1["ur"] >= 0, q2["ur"] >= 0                                   # :517, :523
        a1, b1 = (q1["u"] - c1["cx"]) / c1["fx"], (q1["v"] - c1["cy"]) / c1["fy"]  # :579 Pinhole.cpp:61-64
        a2, b2 = (q2["u"] - c2["cx"]) / c2["fx"], (q2["v"] - c2["cy"]) / c2["fy"]  # :580
        o = np.full(m, one)
        r1 = [dot3((T1[0, i], T1[1, i], T1[2, i]), (a1, b1, o)) for i in range(3)]  # :582 Rwc1 * xn1
        r2 = [dot3((T2[0, i], T2[1, i], T2[2, i]), (a2, b2, o)) for i in range(3)]  # :583
        cos_rays = dot3(r1, r2) / (np.sqrt(dot3(r1, r1)) * np.sqrt(dot3(r2, r2)))   # :584
        cos_base = cos_rays + one                                                # :586
        if exact:
            s1v, s2v = cos_stereo32(g1["mb"], f1["depth"]), cos_stereo32(g2["mb"], f2["depth"])
        else:
            s1v = np.cos(2 * np.arctan2(np.float64(np.float32(g1["mb"]) / np.float32(2)), q1["depth"]))
            s2v = np.cos(2 * np.arctan2(np.float64(np.float32(g2["mb"]) / np.float32(2)), q2["depth"]))
        cs1 = np.where(st1, s1v, cos_base)                                       # :590-591
        cs2 = np.where(~st1 & st2, s2v, cos_base)                                # :592-593
        cos_stereo = np.where(cs2 < cs1, cs2, cs1)                               # :597
        bound = 0.9996 if inertial else 0.9998
        tri = (cos_rays < cos_stereo) & (cos_rays > 0) & (st1 | st2 | (cos_rays.astype(np.float64) < bound))   # :603-604
        arm1 = ~tri & st1 & (cs1 < cs2)                                          # :610
        arm2 = ~tri & ~arm1 & st2 & (cs2 < cs1)                                  # :616
        low = ~tri & ~arm1 & ~arm2                                               # :624
        everyone = np.ones(m, bool)
        comps["parallax_vs_stereo"] = (cos_rays, cos_stereo, one, everyone)
        comps["parallax_vs_zero"] = (cos_rays, 0 * o, one, everyone)
        comps["parallax_vs_bound"] = (cos_rays, bound * o, one, ~st1 & ~st2)
        comps["stereo_order"] = (cs1, cs2, one, ~tri & (st1 | st2))
        # GeometricTools.cc:50-53 in float either way
        f32 = np.float32
        A = np.zeros((m, 4, 4), f32)
        t1f, t2f = np.asarray(g1["Tcw"], f32), np.asarray(g2["Tcw"], f32)
        a1f, b1f = (f1["u"] - f32(g1["cx"])) / f32(g1["fx"]), (f1["v"] - f32(g1["cy"])) / f32(g1["fy"])
        a2f, b2f = (f2["u"] - f32(g2["cx"])) / f32(g2["fx"]), (f2["v"] - f32(g2["cy"])) / f32(g2["fy"])
        A[:, 0, :] = a1f[:, None] * t1f[2][None, :] - t1f[0][None, :]
        A[:, 1, :] = b1f[:, None] * t1f[2][None, :] - t1f[1][None, :]
        A[:, 2, :] = a2f[:, None] * t2f[2][None, :] - t2f[0][None, :]
        A[:, 3, :] = b2f[:, None] * t2f[2][None, :] - t2f[1][None, :]
        xh = np.zeros((m, 4), F)
        if tri.any():
            if exact:
                xh[tri] = jacobi_null_vector32(A[tri])
            else:
                xh[tri] = np.linalg.svd(A[tri].astype(np.float64))[2][:, 3, :]
        null_w = tri & (xh[:, 3] == 0)                                           # GeometricTools.cc:59
        X = np.zeros((m, 3), F)
        X[tri] = xh[tri, :3] / xh[tri, 3:4]                                      # GeometricTools.cc:63

        def unproject(T, O, c, q):                                               # KeyFrame.cc:858-865
            zz = q["depth"]
            x, y = (q["u"] - c["cx"]) * zz * c["invfx"], (q["v"] - c["cy"]) * zz * c["invfy"]
            return np.stack([dot3((T[0, i], T[1, i], T[2, i]), (x, y, zz)) + O[i] for i in range(3)], 1)

        X[arm1] = unproject(T1, O1, c1, q1)[arm1]
        X[arm2] = unproject(T2, O2, c2, q2)[arm2]
        no_depth = (arm1 & ~(q1["depth"] > 0)) | (arm2 & ~(q2["depth"] > 0))     # KeyFrame.cc:856 -> :630
        Xc = (X[:, 0], X[:, 1], X[:, 2])
        z1 = dot3(T1[2, :3], Xc) + T1[2, 3]                                      # :634
        z2 = dot3(T2[2, :3], Xc) + T2[2, 3]                                      # :638
        size = np.sqrt(dot3(Xc, Xc)) + one

        def reproj(T, c, q, z, stereo):                                          # :642-668 / :670-693
            x, y = dot3(T[0, :3], Xc) + T[0, 3], dot3(T[1, :3], Xc) + T[1, 3]
            ex, ey = (c["fx"] * x / z + c["cx"]) - q["u"], (c["fy"] * y / z + c["cy"]) - q["v"]
            mono = ex * ex + ey * ey
            invz = (1.0 / z.astype(np.float64)).astype(F)
            u = c["fx"] * x * invz + c["cx"]
            u_r = u - c1["mbf"] * invz                                           # :661 / :686: KeyFrame 1's mbf in both gates
            v = c["fy"] * y * invz + c["cy"]
            ex, ey, er = u - q["u"], v - q["v"], u_r - q["ur"]
            ster = (ex * ex + ey * ey) + er * er
            return (np.where(stereo, ster, mono).astype(np.float64),
                    np.where(stereo, 7.8, 5.991) * np.asarray(q["sigma2"], np.float64))

        e1, lim1 = reproj(T1, c1, q1, z1, st1)
        e2, lim2 = reproj(T2, c2, q2, z2, st2)
        d1v = [Xc[i] - O1[i] for i in range(3)]
        d2v = [Xc[i] - O2[i] for i in range(3)]
        dist1, dist2 = np.sqrt(dot3(d1v, d1v)), np.sqrt(dot3(d2v, d2v))           # :696-700
        ratio_dist, ratio_oct = dist2 / dist1, q1["scale"] / q2["scale"]          # :708-709
        rf = F(ratio_factor)
    status = np.zeros(m, np.uint8)
    alive = np.ones(m, bool)

    def cut(mask, code):
        nonlocal alive
        hit = alive & mask
        status[hit] = code
        alive = alive & ~mask

    cut(low, LOW_PARALLAX)
    cut(null_w, NULL_W)
    cut(no_depth, STEREO_DEPTH)
    comps["z1"] = (z1, 0 * o, size, alive.copy())
    cut(z1 <= 0, BEHIND1)
    comps["z2"] = (z2, 0 * o, size, alive.copy())
    cut(z2 <= 0, BEHIND2)
    comps["reproj1"] = (e1, lim1, np.maximum(lim1, e1), alive.copy())
    cut(e1 > lim1, REPROJ1)
    comps["reproj2"] = (e2, lim2, np.maximum(lim2, e2), alive.copy())
    cut(e2 > lim2, REPROJ2)
    cut((dist1 == 0) | (dist2 == 0), ZERO_DIST)
    if th_far > 0:
        thf = F(np.float32(th_far))
        comps["far1"] = (dist1, thf * o, thf, alive.copy())
        comps["far2"] = (dist2, thf * o, thf, alive & ~(dist1 >= thf))
        cut((dist1 >= thf) | (dist2 >= thf), FAR)
    lo_l, hi_r = ratio_dist * rf, ratio_oct * rf
    comps["ratio_low"] = (lo_l, ratio_oct, np.maximum(lo_l, ratio_oct), alive.copy())
    comps["ratio_high"] = (ratio_dist, hi_r, np.maximum(ratio_dist, hi_r), alive & ~(lo_l < ratio_oct))
    cut((lo_l < ratio_oct) | (ratio_dist > hi_r), SCALE_RATIO)
    status[alive & tri] = TRIANGULATED
    status[alive & arm1] = STEREO1
    status[alive & arm2] = STEREO2
    X[~alive] = 0
    depth1 = np.where(alive, z1, 1).astype(np.float64)
    return status, X, {k: tuple(np.asarray(a, np.float64) if i < 3 else a for i, a in enumerate(v)) for k, v in comps.items()}, depth1


def features_of(kf, idx):
    g, k = kf["geometry"], kf["kps"]
    return dict(u=k["x"][idx].astype(np.float32), v=k["y"][idx].astype(np.float32), ur=g["u_right"][idx], depth=g["depth"][idx],
                sigma2=SIGMA2[k["octave"][idx]], scale=SCALE[k["octave"][idx]])


def search_pair(oracle, sc, k, valid1):
    """SearchForTriangulation (:492) of the current KeyFrame against neighbour k through the oracle"""
    A, B = sc["kfs"][0], sc["kfs"][k + 1]
    if len(A["kps"]) == 0:
        return np.zeros(0, np.int32)
    p = dict(desc1=A["desc"], desc2=B["desc"], valid1=valid1, avail2=sc["avail2"][k],
             stereo1=(A["geometry"]["u_right"] >= 0).astype(np.uint8), stereo2=(B["geometry"]["u_right"] >= 0).astype(np.uint8),
             fv1=A["fv"], fv2=B["fv"], kp1=A["kps"], kp2=B["kps"], scale_factors2=SCALE, level_sigma2_2=SIGMA2,
             F12=sc["F12"][k], ep=sc["ep"][k])
    if len(B["kps"]) == 0:
        return -np.ones(len(A["kps"]), np.int32)
    return np.array(oracle.search_for_triangulation(p, coarse=sc["coarse"], check_orientation=sc["check_orientation"])[1], np.int32)


_ORACLE = None


def _oracle():
    global _ORACLE
    if _ORACLE is None:
        import orb_oracle
        orb_oracle.lib()
        _ORACLE = orb_oracle
    return _ORACLE


def run_loop(sc, F=np.float32, update_masks=True, matches=None, detail=False):
    """:460-731.  matches: None (search through the oracle) or the match12 of every neighbour to take as given.
    -> per neighbour dict(match12, status, x3D, nmatches, n_created [, comparisons, depth1, idx1])"""
    n1 = len(sc["kfs"][0]["kps"])
    valid = sc["valid1"].copy()
    ratio_factor = np.float32(1.5) * SCALE[1]                                    # :454
    out = []
    for k in range(len(sc["kfs"]) - 1):
        m12 = search_pair(_oracle(), sc, k, valid) if matches is None else np.asarray(matches[k], np.int32)
        idx1 = np.nonzero(m12 >= 0)[0]
        idx2 = m12[idx1]
        status, x3d = np.zeros(n1, np.uint8), np.zeros((n1, 3), F)
        r = dict(match12=m12, status=status, x3D=x3d, nmatches=len(idx1), n_created=0)
        if len(idx1):
            st, X, comps, depth1 = pair_math(sc["kfs"][0]["geometry"], sc["kfs"][k + 1]["geometry"], features_of(sc["kfs"][0], idx1),
                                             features_of(sc["kfs"][k + 1], idx2), sc["inertial"], sc["th_far"], ratio_factor, F)
            status[idx1], x3d[idx1] = st, X
            made = (st >= TRIANGULATED) & (st <= STEREO2)
            r["n_created"] = int(made.sum())
            if update_masks:
                valid[idx1[made]] = 0                                            # :722 -> ORBmatcher.cc:1237-1241
            if detail:
                r.update(comparisons=comps, depth1=depth1, idx1=idx1)
        out.append(r)
    return out


def R32(sc, **kw):
    return run_loop(sc, np.float32, True, **kw)


def R64(sc, **kw):
    return run_loop(sc, np.float64, True, **kw)


def stale(sc):
    return run_loop(sc, np.float32, False)


def cam_floats(g):
    """NpCam of new_points_device.h: 23 floats"""
    return np.concatenate([np.asarray(g["Tcw"], np.float32).reshape(12), np.asarray(g["Ow"], np.float32),
                           [g[k] for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")]]).astype(np.float32)


def pairs_file(sc, k, idx1, idx2):
    """the input of tests/new_points_main.cc for the matched pairs (idx1, idx2) of neighbour k"""
    import struct
    f1, f2 = features_of(sc["kfs"][0], idx1), features_of(sc["kfs"][k + 1], idx2)
    feats = np.stack([np.stack([f[q] for q in ("u", "v", "ur", "depth", "sigma2", "scale")], 1) for f in (f1, f2)], 1)
    return (struct.pack("<iiff", len(idx1), int(sc["inertial"]), float(sc["th_far"]), float(np.float32(1.5) * SCALE[1])) +
            cam_floats(sc["kfs"][0]["geometry"]).tobytes() + cam_floats(sc["kfs"][k + 1]["geometry"]).tobytes() +
            np.ascontiguousarray(feats, np.float32).tobytes())


def store_scene(store, sc):
    """adds the scene's KeyFrames to a msorb.KeyFrameStore -> their ids"""
    return [store.add(kf["kps"], kf["desc"], kf["fv"], SCALE, SIGMA2) for kf in sc["kfs"]]


def device_call(sc, ids, valid1=None, neighbours=None):
    """the arguments of KeyFrameStore.create_new_map_points for the scene (neighbours: which of them, default all)"""
    ks = range(len(sc["kfs"]) - 1) if neighbours is None else neighbours
    call = dict(kf1=ids[0], valid1=sc["valid1"] if valid1 is None else valid1, geometry=sc["kfs"][0]["geometry"], coarse=sc["coarse"],
                check_orientation=sc["check_orientation"], inertial=sc["inertial"], th_far=sc["th_far"])
    nbs = [dict(kf2=ids[k + 1], avail2=sc["avail2"][k], geometry=sc["kfs"][k + 1]["geometry"], F12=sc["F12"][k], ep=sc["ep"][k])
           for k in ks]
    return call, nbs


def same_bits(dev, ref):
    """None when a device result equals a restatement's bit for bit, else what differs"""
    if len(dev) != len(ref):
        return "number of neighbours"
    for k, (a, b) in enumerate(zip(dev, ref)):
        for key in ("match12", "status"):
            if not np.array_equal(np.asarray(a[key]), np.asarray(b[key])):
                return "neighbour %d: %s" % (k, key)
        if not np.array_equal(np.ascontiguousarray(a["x3D"], np.float32).view(np.uint32),
                              np.ascontiguousarray(b["x3D"], np.float32).view(np.uint32)):
            return "neighbour %d: x3D bits" % k
        if (a["nmatches"], a["n_created"]) != (b["nmatches"], b["n_created"]):
            return "neighbour %d: counts %r != %r" % (k, (a["nmatches"], a["n_created"]), (b["nmatches"], b["n_created"]))
    return None


# ---------------------------------------------------------------------------------------------------------------------
# how far the float arithmetic is from a decision: R32 against R64 over the scenes with consistent geometry
# ---------------------------------------------------------------------------------------------------------------------
NATURAL = ("plain", "reclaimed", "inertial_far", "coarse_noorient")


def measure_sensitivity(runs):
    """runs: {scene: (scene dict, R32 with detail, R64 with detail)} -> dict(x3d_rel_depth, cos_form_vs_libm, comparisons {name:
    dict(closest, difference)}): the largest |x3D(R32) - x3D(R64)| over the point's depth in KeyFrame 1; the largest
    difference of the rational cosine from numpy's float32 cos(2 arctan2()); per comparison of :603-711, over the pairs that reach
    it, the closest R64's value comes to its threshold and the largest R32 - R64 difference of (value - threshold) among the pairs
    within 1e-2 of the threshold, both relative to the comparison's scale (a wrong match's ill-conditioned triangulation differs
    wildly between the two and is rejected by a wide margin in both: it says nothing about the arithmetic near a threshold)"""
    D, cosd, comp = 0.0, 0.0, {}
    with np.errstate(all="ignore"):
        for sc, r32, r64 in runs.values():
            for kf in sc["kfs"]:
                g = kf["geometry"]
                s = g["u_right"] >= 0
                if s.any():
                    d = g["depth"][s]
                    cosd = max(cosd, float(np.abs(cos_stereo32(g["mb"], d).astype(np.float64) - cos_stereo_libm32(g["mb"], d)).max()))
            for a, b in zip(r32, r64):
                if "idx1" not in a:
                    continue
                made = ((a["status"] >= TRIANGULATED) & (a["status"] <= STEREO2))[a["idx1"]]
                if made.any():
                    dx = np.abs(a["x3D"][a["idx1"]][made].astype(np.float64) - b["x3D"][b["idx1"]][made]).max(1)
                    D = max(D, float((dx / b["depth1"][made]).max()))
                for name, (l64, r64v, s64, reach64) in b["comparisons"].items():
                    l32, r32v, _, reach32 = a["comparisons"][name]
                    c = comp.setdefault(name, dict(closest=np.inf, difference=0.0))
                    margin, diff = np.abs(l64 - r64v) / s64, np.abs((l32 - r32v) - (l64 - r64v)) / s64
                    both = reach64 & reach32 & np.isfinite(margin) & np.isfinite(diff)
                    if both.any():
                        c["closest"] = min(c["closest"], float(margin[both].min()))
                        near = both & (margin < 1e-2)
                        if near.any():
                            c["difference"] = max(c["difference"], float(diff[near].max()))
    return dict(x3d_rel_depth=D, cos_form_vs_libm=cosd, comparisons=comp)


def natural_runs():
    out = {}
    for name in NATURAL:
        sc = SCENES[name]()
        out[name] = (sc, R32(sc, detail=True), R64(sc, detail=True))
    return out


def _round3(x, up):
    """three significant digits, outwards"""
    import math
    if not np.isfinite(x):
        return None
    if x <= 0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(x)) - 2)
    return float("%.3g" % ((math.ceil(x / q) if up else math.floor(x / q)) * q))


if __name__ == "__main__":   # python tests/new_map_points_cases.py > tests/golden/new_map_points_sensitivity.json
    import json
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, "..", "oracle")]
    m = measure_sensitivity(natural_runs())
    rec = dict(note="measured by tests/new_map_points_cases.py over its scenes " + ", ".join(NATURAL) + "; the measured values "
               "rounded outwards to three digits (R64's LAPACK may differ in the last bits between machines)",
               x3d_rel_depth=_round3(m["x3d_rel_depth"], True), cos_form_vs_libm=_round3(m["cos_form_vs_libm"], True),
               comparisons={k: dict(closest=_round3(v["closest"], False), difference=_round3(v["difference"], True))
                            for k, v in sorted(m["comparisons"].items())})
    json.dump(rec, sys.stdout, indent=1)
    sys.stdout.write("\n")
