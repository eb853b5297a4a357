"""Constructed inputs for the device arithmetic whose results never leave the device — glibc_logf as the device compiles it
(the predicted level of Frame::isInFrustum), glibc_sincosf (the steering of the rBRIEF pattern) — and for the comparisons of
frustum_point / local_points_kernel / last_frame_point, placed ON their boundaries with neighbours on both sides.

Everything is built from exactly representable numbers (identity or signed-permutation poses, a camera with fx = fy = 512,
cx = cy = 256, power-of-two depths), so a boundary case sits on its boundary in float arithmetic, not near it.  The oracle is
the reference for every expected value; tests/test_boundary_cases_cpu.py holds the case sets themselves to their purpose
(the read-out is valid for 100 % of its cases, every boundary is flanked by the opposite outcome)."""
import functools

import numpy as np

F32 = np.float32
CAM = dict(fx=512.0, fy=512.0, cx=256.0, cy=256.0, bounds=(0.0, 512.0, 0.0, 512.0), mbf=64.0)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
NLEVELS = 8
SCALE = np.ones(NLEVELS, np.float32)
for _l in range(1, NLEVELS):
    SCALE[_l] = SCALE[_l - 1] * F32(1.2)            # mvScaleFactor as the extractor accumulates it
FRUSTUM_KEYS = ("track_in_view", "proj_x", "proj_y", "proj_xr", "track_depth", "level", "view_cos")


def log_scale(base):
    """log(scaleFactor) as a float: what Frame hands to MapPoint::PredictScale (mfLogScaleFactor = logf(1.2f); the correctly
    rounded value, which is also what glibc's logf returns for 1.2f, 2.0f and 1.1f — test_boundary_cases_cpu.py checks that)"""
    return float(F32(np.log(np.float64(F32(base)))))


LSF_PRODUCT = log_scale(1.2)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def step(x, n):
    """the float n representable values above (n > 0) or below (n < 0) x; crosses zero and the subnormals like nextafter"""
    x = F32(x)
    to = F32(np.inf) if n > 0 else F32(-np.inf)
    for _ in range(abs(n)):
        x = np.nextafter(x, to, dtype=np.float32)
    return x


def same_bits(a, b):
    """bit-exact equality of two arrays, except that a NaN equals any NaN (the x86 and gfx950 default NaNs differ in the sign
    bit, and the reference promises neither)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def frustum(lsf=LSF_PRODUCT, nlevels=NLEVELS, R=None, t=None, Ow=None):
    import msorb
    z = np.zeros(3, np.float32)
    return msorb.Frustum.make(np.eye(3, dtype=np.float32) if R is None else R, z if t is None else t, z if Ow is None else Ow,
                              CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["bounds"], CAM["mbf"], lsf, nlevels)


def keypoints(xy_octave):
    k = np.zeros(len(xy_octave), KP_DTYPE)
    for i, (x, y, o) in enumerate(xy_octave):
        k[i] = (x, y, 31.0 * SCALE[o], 0.0, 50.0, o, -1)
    return k


def descriptor(seed):
    return np.random.Generator(np.random.PCG64(1000 + seed)).integers(0, 256, 32, dtype=np.uint8)


def flipped(d, nbits):
    d = d.copy()
    for b in range(nbits):
        d[b % 32] ^= np.uint8(1 << (b // 32))
    return d


# ---------------------------------------------------------------------------------------------------------------------
# A. logf, read out through the predicted level
# ---------------------------------------------------------------------------------------------------------------------
READOUT_LEVELS = 1 << 25     # no clamp: the level IS the quotient
DEPTH_EXPONENTS = (0, 3, -5, 12)


def predicted_level(oracle, ratio, lsf):
    """ceil(logf(ratio) / lsf) in float, as MapPoint::PredictScale computes it before the conversion and the clamp"""
    return np.ceil(oracle.logf_n(ratio) / F32(lsf))


def log_scale_factors():
    """logf of 1.2f, 2.0f and 1.1f, and the float above logf(1.2f): what a caller gets who takes the logarithm in another
    library (numpy's float32 log returns it, and the suite's other tests pass that value)"""
    return [LSF_PRODUCT, float(step(LSF_PRODUCT, 1)), log_scale(2.0), log_scale(1.1)]


def flip_point(oracle, lsf, k):
    """the largest float x with ceil(logf(x) / lsf) <= k, by bisection on the bit patterns (the level never decreases with x)"""
    lo, hi = int(bits(F32(0.5))), int(bits(F32(1e6)))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if predicted_level(oracle, from_bits(np.array([mid], np.uint32)), lsf)[0] <= k:
            lo = mid
        else:
            hi = mid
    return from_bits(np.uint32(lo))


@functools.lru_cache(maxsize=None)
def _logf_ratios(oracle):
    sets = {}
    around = []
    for lsf in log_scale_factors():
        for k in range(0, 12 + 1):       # levels of an 8- and a 12-level pyramid and the clamp above them
            b = int(bits(flip_point(oracle, lsf, k)))
            around.append(np.arange(b - 32, b + 33, dtype=np.int64))
    sets["flip"] = from_bits(np.unique(np.concatenate(around)).astype(np.uint32))
    lo, hi = int(bits(F32(5.0) / F32(6.0))), int(bits(F32(16.0)))
    lo += 1                               # 5/6 itself rounds below 1 / 1.2f: dist > 1.2f * max_d there
    sets["sweep"] = from_bits(np.arange(lo + 64, hi, 101, dtype=np.int64).astype(np.uint32))
    sets["large"] = from_bits(np.arange(hi, int(bits(F32(np.finfo(np.float32).max))), 10007, dtype=np.int64).astype(np.uint32))
    one = F32(1.0)
    sets["special"] = np.array([one, step(one, -1), step(one, 1), np.finfo(np.float32).max, np.inf], np.float32)
    return sets


def logf_cases(oracle):
    """-> dict(ratio float32 [n], kexp int [n], family str [n]): map points at P = (0, 0, 2^kexp) seen from the origin with
    max_d = ratio * 2^kexp (exact), so max_d / dist is a real division whose quotient is `ratio`.  `tiny`: depth 2^-74, whose
    square is subnormal."""
    s = _logf_ratios(oracle)
    ratio, kexp, fam = [], [], []
    for name in ("flip", "sweep", "large", "special"):
        r = s[name]
        k = np.asarray(DEPTH_EXPONENTS)[np.arange(len(r)) % len(DEPTH_EXPONENTS)]
        k = np.where(r > F32(1e30), -np.abs(k), k)       # ratio * 2^k stays finite
        ratio.append(r); kexp.append(k); fam += [name] * len(r)
    tiny = s["sweep"][::997]
    ratio.append(tiny); kexp.append(np.full(len(tiny), -74)); fam += ["tiny"] * len(tiny)
    return dict(ratio=np.concatenate(ratio).astype(np.float32), kexp=np.concatenate(kexp).astype(np.int64), family=np.array(fam))


def logf_points(ratio, kexp):
    """the isInFrustum inputs of logf_cases: P, normal, max_d, min_d"""
    n = len(ratio)
    depth = np.ldexp(F32(1.0), kexp).astype(np.float32)
    P = np.zeros((n, 3), np.float32)
    P[:, 2] = depth
    N = np.zeros((n, 3), np.float32)
    N[:, 2] = 1.0
    with np.errstate(over="ignore"):
        maxd = (ratio * depth).astype(np.float32)
    return P, N, maxd, np.zeros(n, np.float32)


def readout_groups(oracle, ratio):
    """One group per binade (and sign) of logf(ratio): (log_scale_factor, indices, expected level).  With log_scale_factor = the
    ulp of that binade — negative for negative logarithms — logf / log_scale_factor is the logarithm's significand as an
    integer, ceil leaves it alone, and READOUT_LEVELS does not clamp it: the level is every bit of logf.  logf == 0 and +inf
    (level 0, the latter through the INT_MIN rule) form a group of their own."""
    L = oracle.logf_n(ratio)
    plain = np.isfinite(L) & (L != 0)
    _, e = np.frexp(np.abs(L).astype(np.float64))
    groups = []
    for sign in (1.0, -1.0):
        for ee in np.unique(e[plain & (np.sign(L) == sign)]):
            idx = np.nonzero(plain & (np.sign(L) == sign) & (e == ee))[0]
            ulp = float(np.ldexp(1.0, int(ee) - 24))
            groups.append((sign * ulp, idx, np.rint(np.abs(L[idx]).astype(np.float64) / ulp).astype(np.int64)))
    idx = np.nonzero(~plain)[0]
    if len(idx):
        groups.append((float(np.ldexp(1.0, -24)), idx, np.zeros(len(idx), np.int64)))
    return groups


def minimal_frame():
    """one keypoint in a corner, far from where the read-out points project: msorb_search_local_points needs a frame"""
    return keypoints([(10.0, 10.0, 0)]), descriptor(0)[None, :].copy()


def local_points_table(P, N, maxd, mind, desc=None, visit=None, bad=None, sparsified=None, obs=None):
    m = len(maxd)
    z = np.zeros(m, np.uint8)
    return dict(pos_w=np.ascontiguousarray(P, np.float32), normal=np.ascontiguousarray(N, np.float32),
                max_distance=np.asarray(maxd, np.float32), min_distance=np.asarray(mind, np.float32),
                visit=np.ones(m, np.uint8) if visit is None else np.asarray(visit, np.uint8),
                bad=z if bad is None else np.asarray(bad, np.uint8), sparsified=z if sparsified is None else np.asarray(sparsified, np.uint8),
                desc=np.tile(descriptor(1), (m, 1)) if desc is None else np.ascontiguousarray(desc, np.uint8),
                obs=np.ones(m, np.int32) if obs is None else np.asarray(obs, np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# B. sincosf: the angles
# ---------------------------------------------------------------------------------------------------------------------
FACTOR_PI = F32(np.pi / 180.0)


@functools.lru_cache(maxsize=None)
def sincos_angles(oracle):
    """float32 degrees: [0, 360] at a stride of 257 ulps; +-16 ulps around k * 45 degrees, k = 0..8 (the quadrant switches of reduce_fast, and
    near 0 the 0x398 branch); 0, the smallest subnormal, the angles around angle * factorPI == 2^-12 and == pi/4 (0x3f4); every
    angle cv::fastAtan2 emits for integer moments |m| <= 64."""
    parts = [np.arange(0, int(bits(F32(360.0))) + 1, 257, dtype=np.int64)]
    for k in range(9):
        b = int(bits(F32(45.0 * k)))
        parts.append(np.arange(max(b - 16, 0), b + 17, dtype=np.int64))
    parts.append(np.array([0, 1], np.int64))
    for lim in (F32(2.0) ** -12, F32(np.pi / 4)):
        lo, hi = 0, int(bits(F32(90.0)))       # the largest angle whose float product with factorPI stays below lim
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if from_bits(np.uint32(mid)) * FACTOR_PI < lim:
                lo = mid
            else:
                hi = mid
        parts.append(np.arange(lo - 16, lo + 17, dtype=np.int64))
    ang = from_bits(np.unique(np.concatenate(parts)).astype(np.uint32))
    m = np.arange(-64, 65, dtype=np.float32)
    m01, m10 = np.meshgrid(m, m, indexing="ij")
    at = oracle.fast_atan2_n(m01.ravel(), m10.ravel())
    return np.concatenate([ang, np.unique(at)]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# C. frustum_point: families of rows around a boundary, in CAMERA coordinates, carried to the world by a scene
# ---------------------------------------------------------------------------------------------------------------------
class Scene:
    """A pose whose rotation is a signed permutation (every product exact): Pc[i] = sign[i] * Pw[perm[i]] + t[i]."""

    def __init__(self, name, perm=(0, 1, 2), sign=(1.0, 1.0, 1.0), t=(0.0, 0.0, 0.0), raw=False):
        self.name, self.perm, self.sign, self.raw = name, perm, np.asarray(sign, np.float32), raw
        self.t = np.asarray(t, np.float32)
        self.R = np.zeros((3, 3), np.float32)
        for i in range(3):
            self.R[i, perm[i]] = sign[i]
        self.Ow = np.zeros(3, np.float32)
        for i in range(3):
            self.Ow[perm[i]] = -(self.sign[i] * self.t[i]) + F32(0.0)     # -R^T t (+0: no negative zeros from t = 0)
        if raw:
            self.Ow = np.zeros(3, np.float32)

    def point(self, Pc):
        if self.raw:
            return np.asarray(Pc, np.float32)
        Pw = np.zeros(3, np.float32)
        with np.errstate(invalid="ignore"):
            for i in range(3):
                Pw[self.perm[i]] = self.sign[i] * (F32(Pc[i]) - self.t[i])
        return Pw

    def normal(self, nc):
        if self.raw:
            return np.asarray(nc, np.float32)
        nw = np.zeros(3, np.float32)
        for i in range(3):
            nw[self.perm[i]] = self.sign[i] * F32(nc[i])
        return nw

    def frustum(self, lsf=LSF_PRODUCT, nlevels=NLEVELS):
        return frustum(lsf, nlevels, self.R, self.t, self.Ow)


def scenes():
    return [Scene("identity"),
            Scene("quarter_turn", perm=(1, 0, 2), sign=(-1.0, 1.0, 1.0), t=(0.5, -0.25, 0.0)),   # Rcw = Rz(90 deg), dyadic translation
            Scene("negative_zero_translation", t=(-0.0, -0.0, -0.0), raw=True)]


def _exact_product(factor, target, around):
    """a float m within +-64 ulps of `around` with float(factor * m) == target, or None"""
    for j in range(-64, 65):
        m = step(around, j)
        if F32(factor) * m == F32(target):
            return m
    return None


def frustum_families():
    """-> list of (family, rows); row = dict(Pc, n, max_d, min_d, centre).  A family walks ONE input across a boundary in steps
    of one ulp (the input is stepped, not the compared value: several inputs round to the same u), the centre row sits on it."""
    S = 8
    fams = []
    up = (0.0, 0.0, 1.0)

    def fam(name, rows):
        fams.append((name, rows))

    def row(Pc, n=up, max_d=None, min_d=0.0, centre=False):
        Pc = tuple(F32(v) for v in Pc)
        if max_d is None:
            with np.errstate(all="ignore"):
                max_d = np.sqrt(Pc[0] * Pc[0] + Pc[1] * Pc[1] + Pc[2] * Pc[2])     # ratio ~ 1
        return dict(Pc=Pc, n=tuple(F32(v) for v in n), max_d=F32(max_d), min_d=F32(min_d), centre=centre)

    # image bounds: u = 512 x / 2 + 256 is 512 at x = 1 and 0 at x = -1 (kept: the reference rejects u > max only)
    fam("u_max", [row((step(1.0, j), 0.0, 2.0), centre=j == 0) for j in range(-S, S + 1)])
    fam("u_min", [row((step(-1.0, j), 0.0, 2.0), centre=j == 0) for j in range(-S, S + 1)])
    fam("v_max", [row((0.0, step(1.0, j), 2.0), centre=j == 0) for j in range(-S, S + 1)])
    fam("v_min", [row((0.0, step(-1.0, j), 2.0), centre=j == 0) for j in range(-S, S + 1)])
    # depth around zero: +0 (kept: NaN projections, in view), subnormals of both signs, the first normals
    tiny = [F32(0.0), step(0.0, 1), step(0.0, 2), step(0.0, -1), step(0.0, -2), np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny]
    fam("z_zero", [row((0.0, 0.0, z), max_d=1.0, centre=i == 0) for i, z in enumerate(tiny)] +
        [row((1.0, 0.0, z), max_d=1.0) for z in tiny] + [row((0.0, -1.0, z), max_d=1.0) for z in tiny])
    # distance range: dist = 4 against 0.8f * min_d (min_d = 5 gives exactly 4) and against 1.2f * max_d
    fam("dist_min", [row((0.0, 0.0, 4.0), max_d=6.0, min_d=step(5.0, j), centre=j == 0) for j in range(-S, S + 1)])
    for d in (4.0, 5.0, 6.0, 7.0, 12.0):
        m = _exact_product(1.2, d, F32(d) / F32(1.2))
        centre = F32(d) / F32(1.2) if m is None else m       # no exact product (d = 4): the two adjacent ones are in the walk
        fam("dist_max_%g%s" % (d, "" if m is None else "_exact"),
            [row((0.0, 0.0, d), max_d=step(centre, j), centre=j == 0) for j in range(-S, S + 1)])
    # viewing angle: PO = (0, 0, 2^k), n = (0, 0, c): viewCos = c exactly; equality with the limit is kept
    for k in (0, 3):
        fam("view_cos_2^%d" % k, [row((0.0, 0.0, 2.0 ** k), n=(0.0, 0.0, step(0.5, j)), centre=j == 0) for j in range(-S, S + 1)])
    # the level clamp at both ends, and a walk across every level in between
    ratios = [0.84, 0.9, step(1.0, -1), 1.0, step(1.0, 1)] + [1.2 ** (k + f) for k in range(0, 10) for f in (0.25, 0.75)] + [100.0, 1e30]
    fam("level_clamp", [row((0.0, 0.0, 4.0), max_d=F32(r) * F32(4.0), centre=i == 3) for i, r in enumerate(ratios)])
    # non-finite and degenerate ranges, at a point in view and at the camera centre
    weird = [np.inf, np.nan, 0.0, -0.0, -1.0, -np.inf, step(0.0, 1), np.finfo(np.float32).max]
    fam("max_d_special", [row((0.0, 0.0, 4.0), max_d=4.0, centre=True)] + [row(P, max_d=m) for P in ((0.0, 0.0, 4.0), (0.0, 0.0, 0.0)) for m in weird])
    fam("min_d_special", [row((0.0, 0.0, 4.0), max_d=4.0, min_d=m, centre=i == 2) for i, m in enumerate(weird)])
    nf = [np.nan, np.inf, -np.inf]
    fam("P_special", [row((0.0, 0.0, 4.0), centre=True)] +
        [row(P, max_d=m) for v in nf for P in ((v, 0.0, 4.0), (0.0, v, 4.0), (0.0, 0.0, v), (v, v, v)) for m in (4.0, np.inf)] +
        [row((0.0, 0.0, 4.0), n=n) for n in ((np.nan, 0.0, 1.0), (0.0, 0.0, np.inf), (0.0, 0.0, np.nan))])
    # a map point deeper than the float range of its square, and one whose square is subnormal
    fam("depth_range", [row((0.0, 0.0, 2.0 ** k), max_d=F32(2.0 ** k), centre=k == 0) for k in (0, -74, -75, -76, 63, 64, 100)])
    return fams


def negative_zero_rows():
    """PcZ == -0.0f needs every term of the row AND the translation negative zero: all sign patterns of a zero point, in world
    coordinates, for the scene whose translation is (-0, -0, -0)."""
    rows = []
    for s in range(8):
        P = tuple(F32(-0.0) if s >> i & 1 else F32(0.0) for i in range(3))
        rows.append(dict(Pc=P, n=(F32(0), F32(0), F32(1)), max_d=F32(1.0), min_d=F32(0.0), centre=s == 7))
    return [("z_negative_zero", rows)]


def frustum_scene_cases(scene):
    """-> (table for msorb_is_in_frustum / msorb_search_local_points, family name per row, centre flag per row)"""
    fams = negative_zero_rows() if scene.raw else frustum_families()
    P, N, mx, mn, names, centre = [], [], [], [], [], []
    for name, rows in fams:
        for r in rows:
            P.append(scene.point(r["Pc"])); N.append(scene.normal(r["n"])); mx.append(r["max_d"]); mn.append(r["min_d"])
            names.append(name); centre.append(r["centre"])
    m = len(mx)
    rng = np.random.Generator(np.random.PCG64(5))
    tab = local_points_table(np.array(P, np.float32).reshape(m, 3), np.array(N, np.float32).reshape(m, 3), np.array(mx, np.float32),
                             np.array(mn, np.float32), desc=rng.integers(0, 256, (m, 32), dtype=np.uint8))
    return tab, np.array(names), np.array(centre, bool)


def outcome(r, i):
    """what the comparisons decided for row i of an isInFrustum result: in view?, projected?, level"""
    return (int(r["track_in_view"][i]), bool(r["proj_x"][i] != -1.0), int(r["level"][i]))


# ---------------------------------------------------------------------------------------------------------------------
# C. local_points_kernel only: what the kernel decides AFTER the frustum test is seen through the matches, so every variant
# is one call on a frame of a handful of keypoints placed where the decision moves one of them in or out of the window
# ---------------------------------------------------------------------------------------------------------------------
def local_points_variants():
    """-> list of dict(case, variant, kps, desc, mp, th, far, th_far, frame_mp); the variants of a case differ in ONE input and
    must not all give the same matches (tests/test_boundary_cases_cpu.py)."""
    D = descriptor(2)
    out = []

    def add(case, variant, kps, kdesc, mp, th=1.0, far=False, th_far=50.0, frame_mp=None):
        out.append(dict(case=case, variant=variant, kps=kps, desc=np.ascontiguousarray(kdesc, np.uint8), mp=mp, th=float(th), far=far,
                        th_far=float(th_far), frame_mp=np.full(len(kps), -1, np.int32) if frame_mp is None else np.asarray(frame_mp, np.int32)))

    def one_point(P, n=(0.0, 0.0, 1.0), max_d=None, **kw):
        P = np.array([P], np.float32)
        d = np.sqrt((P.astype(np.float32) ** 2).sum(dtype=np.float32)) if max_d is None else F32(max_d)
        return local_points_table(P, np.array([n], np.float32), np.array([d], np.float32), np.zeros(1, np.float32), desc=D[None, :], **kw)

    # RadiusByViewingCos: (double)viewCos > 0.998.  float(0.998) is above the double, its predecessor below: radius 2.5 / 4 at
    # level 0, a keypoint 3 pixels from the projection
    c998 = F32(0.998)
    for name, c in (("below", step(c998, -1)), ("float_0.998", c998), ("above", step(c998, 1))):
        add("view_cos_0.998", name, keypoints([(259.0, 256.0, 0)]), D[None, :], one_point((0.0, 0.0, 4.0), n=(0.0, 0.0, c)))
    # th == 1.0f: the radius 4 * th at level 0 around u = 0; keypoints at x = 4 (an exact copy) and at the float below 4
    kp2 = keypoints([(step(4.0, -1), 256.0, 0), (4.0, 256.0, 0)])
    d2 = np.stack([flipped(D, 10), D])
    for name, th in (("below", step(1.0, -1)), ("one", F32(1.0)), ("above", step(1.0, 1))):
        add("th_one", name, kp2, d2, one_point((-1.0, 0.0, 2.0)), th=th)
    # bFarPoints && mTrackDepth > thFarPoints, depth = 8 exactly
    kp1 = keypoints([(256.0, 256.0, 0)])
    for name, far, tf in (("equal", True, F32(8.0)), ("below", True, step(8.0, -1)), ("below_but_off", False, step(8.0, -1))):
        add("th_far", name, kp1, D[None, :], one_point((0.0, 0.0, 8.0)), far=far, th_far=tf)
    # the flags.  Point 0 is behind the camera and holds the keypoint in the `occupied` variants
    def two_points(**kw):
        P = np.array([(0.0, 0.0, -5.0), (0.0, 0.0, 4.0)], np.float32)
        return local_points_table(P, np.array([(0.0, 0.0, 1.0)] * 2, np.float32), np.array([5.0, 4.0], np.float32), np.zeros(2, np.float32),
                                  desc=np.stack([D, D]), obs=np.array([5, 1], np.int32), **kw)
    add("flags", "plain", kp1, D[None, :], two_points())
    add("flags", "not_visited", kp1, D[None, :], two_points(visit=[1, 0]))
    add("flags", "bad", kp1, D[None, :], two_points(bad=[0, 1]))
    add("flags", "occupied", kp1, D[None, :], two_points(), frame_mp=[0])
    add("flags", "occupied_sparsified", kp1, D[None, :], two_points(sparsified=[0, 1]), frame_mp=[0])
    # the level band [level - 1, level]: level 0 gives min_level = -1.  (point level, keypoint octave) per site
    pairs = [(0, 0), (0, 1), (1, 0), (1, 2), (2, 0), (2, 1), (7, 6), (7, 5)]
    sites = [(32.0 + 64.0 * i, 128.0) for i in range(len(pairs))]
    P = np.array([((u - 256.0) * 4.0 / 512.0, (v - 256.0) * 4.0 / 512.0, 4.0) for u, v in sites], np.float32)
    dist = np.sqrt((P.astype(np.float64) ** 2).sum(1))
    maxd = (dist * np.array([1.2 ** lv for lv, _ in pairs]) * 0.95).astype(np.float32)
    descs = np.stack([descriptor(10 + i) for i in range(len(pairs))])
    mp = local_points_table(P, np.tile(np.array([(0.0, 0.0, 1.0)], np.float32), (len(pairs), 1)), maxd, np.zeros(len(pairs), np.float32), desc=descs)
    add("level_band", "all", keypoints([(u, v, o) for (u, v), (_, o) in zip(sites, pairs)]), descs, mp)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# C. last_frame_point (TrackWithMotionModel's projection), through msorb_search_last_frame(want_projection)
# ---------------------------------------------------------------------------------------------------------------------
def _last_table(P, octave=None, desc=None, has_point=None):
    n = len(P)
    return dict(has_point=np.ones(n, np.uint8) if has_point is None else np.asarray(has_point, np.uint8),
                pos_w=np.ascontiguousarray(P, np.float32).reshape(n, 3), octave=np.zeros(n, np.int32) if octave is None else np.asarray(octave, np.int32),
                angle=np.zeros(n, np.float32), desc=np.tile(descriptor(3), (n, 1)) if desc is None else np.ascontiguousarray(desc, np.uint8),
                obs=np.ones(n, np.int32))


def last_frame_edge_rows():
    """world points (identity pose) on the boundaries of the projection: the image bounds, depth zero of both magnitudes"""
    S = 8
    rows, names, centre = [], [], []

    def fam(name, pts, c):
        for i, p in enumerate(pts):
            rows.append(p); names.append(name); centre.append(i == c)

    fam("u_max", [(step(1.0, j), 0.0, 2.0) for j in range(-S, S + 1)], S)
    fam("u_min", [(step(-1.0, j), 0.0, 2.0) for j in range(-S, S + 1)], S)
    fam("v_max", [(0.0, step(1.0, j), 2.0) for j in range(-S, S + 1)], S)
    fam("v_min", [(0.0, step(-1.0, j), 2.0) for j in range(-S, S + 1)], S)
    tiny = [F32(0.0), step(0.0, 1), step(0.0, -1), step(0.0, 2), step(0.0, -2), np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny]
    fam("z_zero", [(0.0, 0.0, z) for z in tiny] + [(1.0, 0.0, z) for z in tiny] + [(0.0, -1.0, z) for z in tiny], 0)
    fam("P_special", [(0.0, 0.0, 4.0), (0.0, 0.0, -4.0), (4.0, 0.0, 1.0)] + [p for v in (np.nan, np.inf, -np.inf) for p in ((v, 0.0, 4.0), (0.0, 0.0, v), (v, v, v))], 0)
    return np.array(rows, np.float32), np.array(names), np.array(centre, bool)


def last_frame_calls():
    """-> list of dict(case, variant, q, t, forward, backward, last, kps, desc, th, names, centre)"""
    calls = []
    ident = (0.0, 0.0, 0.0, 1.0)
    kp0, d0 = minimal_frame()

    def add(case, variant, q, t, last, kps=kp0, desc=d0, forward=False, backward=False, th=7.0, names=None, centre=None):
        calls.append(dict(case=case, variant=variant, q=tuple(float(F32(v)) for v in q), t=tuple(float(F32(v)) for v in t), last=last, kps=kps,
                          desc=np.ascontiguousarray(desc, np.uint8), forward=forward, backward=backward, th=float(th), names=names, centre=centre))

    P, names, centre = last_frame_edge_rows()
    add("edges", "identity", ident, (0.0, 0.0, 0.0), _last_table(P), names=names, centre=centre)
    # a dyadic rotation: the quaternion of Rz(180 deg) is (0, 0, 1, 0); the translation puts the rotated points back
    add("edges", "half_turn", (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0), _last_table(P * np.array([-1.0, -1.0, 1.0], np.float32)), names=names, centre=centre)
    add("edges", "translated", ident, (0.5, -0.25, 1.0),
        _last_table(np.where(np.isfinite(P), P - np.array([0.5, -0.25, 1.0], np.float32), P)[names != "z_zero"]), names=names[names != "z_zero"],
        centre=centre[names != "z_zero"])
    # zc == -0.0f: invzc = -inf is rejected, +0 is not.  A sum of zeros is -0 only if every term is: with q.w = 1 some term of the
    # quaternion action is always +0, with the same rotation written as q = (-0, 0, 0, -1) and t.z = -0 the point (0, -0, -0)
    # gets there.  Every sign pattern of a zero point, under both
    zeros = [tuple(-0.0 if s >> i & 1 else 0.0 for i in range(3)) for s in range(8)]
    for variant, q, t in (("w_plus_one", ident, (0.0, 0.0, 0.0)), ("w_minus_one", (-0.0, 0.0, 0.0, -1.0), (0.0, 0.0, -0.0))):
        add("z_signed_zero", variant, q, t, _last_table(np.array(zeros, np.float32)), names=np.array(["z_signed_zero"] * 8),
            centre=np.arange(8) == 6)
    # table sizes around the block sizes of the kernels that carry the projection (256 threads; 1024 in the grid launch)
    for n in (1, 63, 64, 65, 1025):
        idx = np.arange(n) % len(P)
        add("table_size", str(n), ident, (0.0, 0.0, 0.0), _last_table(P[idx]), names=names[idx], centre=centre[idx])
    # the level band of the window: octave 0 and the top octave, forward / backward / neither
    pairs = [(po, ko) for po in (0, NLEVELS - 1) for ko in (0, 1, NLEVELS - 2, NLEVELS - 1)]
    sites = [(32.0 + 64.0 * (i % 4), 128.0 + 256.0 * (i // 4)) for i in range(len(pairs))]
    Pb = np.array([((u - 256.0) * 4.0 / 512.0, (v - 256.0) * 4.0 / 512.0, 4.0) for u, v in sites], np.float32)
    descs = np.stack([descriptor(20 + i) for i in range(len(pairs))])
    kb = keypoints([(u, v, ko) for (u, v), (_, ko) in zip(sites, pairs)])
    for variant, fw, bw in (("neither", False, False), ("forward", True, False), ("backward", False, True)):
        add("level_band", variant, ident, (0.0, 0.0, 0.0), _last_table(Pb, octave=[po for po, _ in pairs], desc=descs), kps=kb, desc=descs,
            forward=fw, backward=bw)
    return calls
