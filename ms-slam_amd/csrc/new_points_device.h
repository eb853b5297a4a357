// The body of the match loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:578-712) for ONE matched pair of two pinhole
// KeyFrames without a second camera: parallax test, GeometricTools::Triangulate (GeometricTools.cc:47-66) or
// KeyFrame::UnprojectStereo (KeyFrame.cc:852-870), the two depth tests, the two reprojection gates, the scale-consistency gate.
// One statement of the arithmetic for the device (new_points_kernel, bow_match.hip) and the host (tests/new_points_main.cc):
// every float operation is a single correctly rounded IEEE operation in the reference's statement order, products summed
// left to right, nothing contracted.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NP_HD __host__ __device__ __forceinline__
#define NP_UNROLL _Pragma("unroll")
#else
#include <math.h>
#define NP_HD inline
#define NP_UNROLL
#endif

namespace msorb {

#if defined(__HIP_DEVICE_COMPILE__)
NP_HD float np_mul(float a, float b) { return __fmul_rn(a, b); }
NP_HD float np_add(float a, float b) { return __fadd_rn(a, b); }
NP_HD float np_sub(float a, float b) { return __fsub_rn(a, b); }
NP_HD float np_div(float a, float b) { return __fdiv_rn(a, b); }
NP_HD float np_sqrt(float a) { return sqrtf(a); }   // correctly rounded in hipcc's default mode; __fsqrt_rn is the bare 1-ulp v_sqrt_f32
NP_HD double np_dmul(double a, double b) { return __dmul_rn(a, b); }
NP_HD double np_dadd(double a, double b) { return __dadd_rn(a, b); }
NP_HD double np_dsub(double a, double b) { return __dsub_rn(a, b); }
NP_HD double np_ddiv(double a, double b) { return __ddiv_rn(a, b); }
#else   // host: built with -ffp-contract=off
NP_HD float np_mul(float a, float b) { return a * b; }
NP_HD float np_add(float a, float b) { return a + b; }
NP_HD float np_sub(float a, float b) { return a - b; }
NP_HD float np_div(float a, float b) { return a / b; }
NP_HD float np_sqrt(float a) { return sqrtf(a); }
NP_HD double np_dmul(double a, double b) { return a * b; }
NP_HD double np_dadd(double a, double b) { return a + b; }
NP_HD double np_dsub(double a, double b) { return a - b; }
NP_HD double np_ddiv(double a, double b) { return a / b; }
#endif
NP_HD float np_abs(float a) { return fabsf(a); }
NP_HD float np_max(float a, float b) { return b > a ? b : a; }
// a*x + b*y and a*x - b*y: two rounded products, one rounded sum
NP_HD float np_axpby(float a, float x, float b, float y) { return np_add(np_mul(a, x), np_mul(b, y)); }
NP_HD float np_axmby(float a, float x, float b, float y) { return np_sub(np_mul(a, x), np_mul(b, y)); }
// (a0*b0 + a1*b1) + a2*b2
NP_HD float np_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return np_add(np_add(np_mul(a0, b0), np_mul(a1, b1)), np_mul(a2, b2));
}

// One byte per query of KeyFrame 1 and neighbour: what became of it.
enum NewPointStatus : uint8_t {
    kNpNone = 0,            // not matched
    kNpTriangulated = 1,    // created by GeometricTools::Triangulate (:606)
    kNpStereo1 = 2,         // created from KeyFrame 1's stereo measurement (:614)
    kNpStereo2 = 3,         // created from KeyFrame 2's stereo measurement (:620)
    kNpLowParallax = 4,     // :624 no stereo and very low parallax
    kNpNullW = 5,           // :607-608 x3Dh(3) == 0
    kNpStereoDepth = 6,     // :630-631 UnprojectStereo refused (depth <= 0)
    kNpBehind1 = 7,         // :635 z1 <= 0
    kNpBehind2 = 8,         // :639 z2 <= 0
    kNpReproj1 = 9,         // :654 / :666
    kNpReproj2 = 10,        // :680 / :691
    kNpZeroDist = 11,       // :702
    kNpFar = 12,            // :705
    kNpScaleRatio = 13,     // :711
};

struct NpCam {      // one KeyFrame's geometry
    float T[12];    // Tcw, 3x4 row major
    float Ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
};

struct NpFeature {  // one keypoint of a matched pair
    float u, v;     // GetKeyPoint(idx).pt
    float ur;       // GetuRight(idx): stereo when >= 0
    float depth;    // GetDepth(idx)
    float sigma2;   // mvLevelSigma2[octave]
    float scale;    // mvScaleFactors[octave]
};

constexpr int kNpMaxSweeps = 60;   // Jacobi sweeps: a 4x4 matrix converges in < 10; the bound keeps a lane from spinning on garbage

// The right singular vector of A's (4x4, row major) smallest singular value the way Eigen::JacobiSVD<Matrix4f> reaches it, as far as
// that algorithm is publicly described: A scaled by its largest |entry|, two-sided Jacobi over the sub-problems (p, q), p = 1..3,
// q = 0..p-1, a 2x2 block rotated when |W(p,q)| or |W(q,p)| exceeds max(FLT_MIN, 2 eps maxDiag) (real_2x2_jacobi_svd: a rotation
// that makes the block symmetric, then the Jacobi rotation that diagonalises it), sweeps until one passes with no rotation, then the
// singular values |W(i,i)| put in descending order by selection with swaps, V's columns following.  x = V.col(3).
NP_HD void np_null_vector(const float* A, float* x) {
    const float tiny = 1.17549435e-38f, precision = 2.384185791015625e-07f;   // FLT_MIN, 2 * FLT_EPSILON
    float W[4][4], V[4][4];
    float scale = 0.0f;
NP_UNROLL
    for (int i = 0; i < 16; i++) scale = np_max(scale, np_abs(A[i]));
    if (scale == 0.0f) scale = 1.0f;
NP_UNROLL
    for (int i = 0; i < 4; i++)
NP_UNROLL
        for (int j = 0; j < 4; j++) { W[i][j] = np_div(A[4 * i + j], scale); V[i][j] = i == j ? 1.0f : 0.0f; }
    float max_diag = np_max(np_max(np_abs(W[0][0]), np_abs(W[1][1])), np_max(np_abs(W[2][2]), np_abs(W[3][3])));
    for (int sweep = 0; sweep < kNpMaxSweeps; sweep++) {
        bool finished = true;
NP_UNROLL
        for (int p = 1; p < 4; p++)
NP_UNROLL
            for (int q = 0; q < p; q++) {
                const float thr = np_max(tiny, np_mul(precision, max_diag));
                if (!(np_abs(W[p][q]) > thr || np_abs(W[q][p]) > thr)) continue;
                finished = false;
                // real_2x2_jacobi_svd on [W(p,p) W(p,q); W(q,p) W(q,q)]
                const float m00 = W[p][p], m01 = W[p][q], m10 = W[q][p], m11 = W[q][q];
                const float t = np_add(m00, m11), d = np_sub(m10, m01);
                float c1 = 1.0f, s1 = 0.0f;
                if (!(np_abs(d) < tiny)) {
                    const float u = np_div(t, d), tmp = np_sqrt(np_add(1.0f, np_mul(u, u)));
                    s1 = np_div(1.0f, tmp);
                    c1 = np_div(u, tmp);
                }
                const float n00 = np_axpby(c1, m00, s1, m10), n01 = np_axpby(c1, m01, s1, m11), n11 = np_axmby(c1, m11, s1, m01);
                float cr = 1.0f, sr = 0.0f;   // makeJacobi(n00, n01, n11)
                const float deno = np_mul(2.0f, np_abs(n01));
                if (!(deno < tiny)) {
                    const float tau = np_div(np_sub(n00, n11), deno), w = np_sqrt(np_add(np_mul(tau, tau), 1.0f));
                    const float tt = tau > 0.0f ? np_div(1.0f, np_add(tau, w)) : np_div(1.0f, np_sub(tau, w));
                    const float n = np_div(1.0f, np_sqrt(np_add(np_mul(tt, tt), 1.0f)));
                    const float mag = np_mul(np_abs(tt), n);
                    sr = ((tt > 0.0f) == (n01 > 0.0f)) ? -mag : mag;   // -sign(t) * (y / |y|) * |t| * n
                    cr = n;
                }
                const float cl = np_axpby(c1, cr, s1, sr), sl = np_axmby(s1, cr, c1, sr);   // rot1 * j_right.transpose()
NP_UNROLL
                for (int k = 0; k < 4; k++) {   // W.applyOnTheLeft(p, q, j_left)
                    const float a = W[p][k], b = W[q][k];
                    W[p][k] = np_axpby(cl, a, sl, b);
                    W[q][k] = np_axmby(cl, b, sl, a);
                }
NP_UNROLL
                for (int k = 0; k < 4; k++) {   // W.applyOnTheRight(p, q, j_right), V.applyOnTheRight(p, q, j_right)
                    const float a = W[k][p], b = W[k][q];
                    W[k][p] = np_axmby(cr, a, sr, b);
                    W[k][q] = np_axpby(sr, a, cr, b);
                    const float va = V[k][p], vb = V[k][q];
                    V[k][p] = np_axmby(cr, va, sr, vb);
                    V[k][q] = np_axpby(sr, va, cr, vb);
                }
                max_diag = np_max(max_diag, np_max(np_abs(W[p][p]), np_abs(W[q][q])));
            }
        if (finished) break;
    }
    // descending order by selection: position i takes the first maximum of positions i..3 (a swap), and stops at a zero maximum
    float sv[4];
    int col[4];
NP_UNROLL
    for (int i = 0; i < 4; i++) { sv[i] = np_abs(W[i][i]); col[i] = i; }
    bool stop = false;
NP_UNROLL
    for (int i = 0; i < 4; i++) {
        float best = sv[i];
        int pos = i;
NP_UNROLL
        for (int k = i + 1; k < 4; k++)
            if (sv[k] > best) { best = sv[k]; pos = k; }
        if (best == 0.0f) stop = true;
NP_UNROLL
        for (int k = i + 1; k < 4; k++)
            if (!stop && k == pos) {
                const float ts = sv[i]; sv[i] = sv[k]; sv[k] = ts;
                const int tc = col[i]; col[i] = col[k]; col[k] = tc;
            }
    }
    const int last = col[3];
NP_UNROLL
    for (int i = 0; i < 4; i++) x[i] = last == 0 ? V[i][0] : last == 1 ? V[i][1] : last == 2 ? V[i][2] : V[i][3];
}

// cos(2 * atan2(h, d)) = (d^2 - h^2) / (d^2 + h^2) with h = mb / 2 (a float), in double from the float inputs, narrowed once
// (:591, :593; departs from libm's cosf(2 * atan2f()) by rounding only: DESIGN.md section 11)
NP_HD float np_cos_stereo(float mb, float depth) {
    const double h = (double)np_div(mb, 2.0f), d = (double)depth;
    const double hh = np_dmul(h, h), dd = np_dmul(d, d);
    return (float)np_ddiv(np_dsub(dd, hh), np_dadd(dd, hh));
}

// sum of squares promoted to double against chi2 * sigma2 in double (:654, :666, :680, :691)
NP_HD bool np_gate_exceeds(float sum, double chi2, float sigma2) { return (double)sum > np_dmul(chi2, (double)sigma2); }

// one KeyFrame's reprojection gate (:642-668 for KeyFrame 1, :670-693 for KeyFrame 2); mbf is KeyFrame 1's in both
NP_HD bool np_reprojection_fails(const NpCam& c, const NpFeature& f, const float* X, float z, float mbf) {
    const float x = np_add(np_dot3(c.T[0], c.T[1], c.T[2], X[0], X[1], X[2]), c.T[3]);
    const float y = np_add(np_dot3(c.T[4], c.T[5], c.T[6], X[0], X[1], X[2]), c.T[7]);
    if (!(f.ur >= 0.0f)) {   // pCamera->project (Pinhole.cpp:30-33)
        const float ex = np_sub(np_add(np_div(np_mul(c.fx, x), z), c.cx), f.u);
        const float ey = np_sub(np_add(np_div(np_mul(c.fy, y), z), c.cy), f.v);
        return np_gate_exceeds(np_add(np_mul(ex, ex), np_mul(ey, ey)), 5.991, f.sigma2);
    }
    const float invz = (float)np_ddiv(1.0, (double)z);   // const float invz = 1.0 / z
    const float u = np_add(np_mul(np_mul(c.fx, x), invz), c.cx);
    const float u_r = np_sub(u, np_mul(mbf, invz));
    const float v = np_add(np_mul(np_mul(c.fy, y), invz), c.cy);
    const float ex = np_sub(u, f.u), ey = np_sub(v, f.v), er = np_sub(u_r, f.ur);
    return np_gate_exceeds(np_add(np_add(np_mul(ex, ex), np_mul(ey, ey)), np_mul(er, er)), 7.8, f.sigma2);
}

// mRwc * x3Dc + Ow of KeyFrame::UnprojectStereo (KeyFrame.cc:858-865); false: depth <= 0
NP_HD bool np_unproject_stereo(const NpCam& c, const NpFeature& f, float* X) {
    const float z = f.depth;
    if (!(z > 0.0f)) return false;
    const float x = np_mul(np_mul(np_sub(f.u, c.cx), z), c.invfx), y = np_mul(np_mul(np_sub(f.v, c.cy), z), c.invfy);
NP_UNROLL
    for (int i = 0; i < 3; i++) X[i] = np_add(np_dot3(c.T[i], c.T[4 + i], c.T[8 + i], x, y, z), c.Ow[i]);   // Rwc = Rcw^T
    return true;
}

// :578-712 for one pair.  Returns the status; X is defined when the status is one of the three "created".
NP_HD uint8_t new_point_pair(const NpCam& c1, const NpCam& c2, const NpFeature& f1, const NpFeature& f2, int inertial, float th_far,
                             float ratio_factor, float* X) {
    const bool stereo1 = f1.ur >= 0.0f, stereo2 = f2.ur >= 0.0f;   // :517, :523 (no second camera)
    // :579-584 unprojectEig (Pinhole.cpp:61-64), ray = Rwc * xn, the cosine as dot / (norm1 * norm2)
    const float a1 = np_div(np_sub(f1.u, c1.cx), c1.fx), b1 = np_div(np_sub(f1.v, c1.cy), c1.fy);
    const float a2 = np_div(np_sub(f2.u, c2.cx), c2.fx), b2 = np_div(np_sub(f2.v, c2.cy), c2.fy);
    float r1[3], r2[3];
NP_UNROLL
    for (int i = 0; i < 3; i++) {
        r1[i] = np_dot3(c1.T[i], c1.T[4 + i], c1.T[8 + i], a1, b1, 1.0f);
        r2[i] = np_dot3(c2.T[i], c2.T[4 + i], c2.T[8 + i], a2, b2, 1.0f);
    }
    const float n1 = np_sqrt(np_dot3(r1[0], r1[1], r1[2], r1[0], r1[1], r1[2]));
    const float n2 = np_sqrt(np_dot3(r2[0], r2[1], r2[2], r2[0], r2[1], r2[2]));
    const float cos_rays = np_div(np_dot3(r1[0], r1[1], r1[2], r2[0], r2[1], r2[2]), np_mul(n1, n2));
    // :586-597
    const float cos_base = np_add(cos_rays, 1.0f);
    float cs1 = cos_base, cs2 = cos_base;
    if (stereo1) cs1 = np_cos_stereo(c1.mb, f1.depth);
    else if (stereo2) cs2 = np_cos_stereo(c2.mb, f2.depth);
    const float cos_stereo = cs2 < cs1 ? cs2 : cs1;   // std::min(cs1, cs2)
    uint8_t made;
    // :603-625
    if (cos_rays < cos_stereo && cos_rays > 0.0f &&
        (stereo1 || stereo2 || (inertial ? (double)cos_rays < 0.9996 : (double)cos_rays < 0.9998))) {
        float A[16], xh[4];   // GeometricTools.cc:50-53
NP_UNROLL
        for (int k = 0; k < 4; k++) {
            A[k] = np_sub(np_mul(a1, c1.T[8 + k]), c1.T[k]);
            A[4 + k] = np_sub(np_mul(b1, c1.T[8 + k]), c1.T[4 + k]);
            A[8 + k] = np_sub(np_mul(a2, c2.T[8 + k]), c2.T[k]);
            A[12 + k] = np_sub(np_mul(b2, c2.T[8 + k]), c2.T[4 + k]);
        }
        np_null_vector(A, xh);
        if (xh[3] == 0.0f) return kNpNullW;
NP_UNROLL
        for (int i = 0; i < 3; i++) X[i] = np_div(xh[i], xh[3]);
        made = kNpTriangulated;
    } else if (stereo1 && cs1 < cs2) {
        if (!np_unproject_stereo(c1, f1, X)) return kNpStereoDepth;
        made = kNpStereo1;
    } else if (stereo2 && cs2 < cs1) {
        if (!np_unproject_stereo(c2, f2, X)) return kNpStereoDepth;
        made = kNpStereo2;
    } else {
        return kNpLowParallax;
    }
    // :634-640
    const float z1 = np_add(np_dot3(c1.T[8], c1.T[9], c1.T[10], X[0], X[1], X[2]), c1.T[11]);
    if (z1 <= 0.0f) return kNpBehind1;
    const float z2 = np_add(np_dot3(c2.T[8], c2.T[9], c2.T[10], X[0], X[1], X[2]), c2.T[11]);
    if (z2 <= 0.0f) return kNpBehind2;
    if (np_reprojection_fails(c1, f1, X, z1, c1.mbf)) return kNpReproj1;
    // u2_r = u2 - mpCurrentKeyFrame->mbf * invz2 (:686): KeyFrame 1's mbf in KeyFrame 2's gate, as the reference has it
    if (np_reprojection_fails(c2, f2, X, z2, c1.mbf)) return kNpReproj2;
    // :696-712
    const float e0 = np_sub(X[0], c1.Ow[0]), e1 = np_sub(X[1], c1.Ow[1]), e2 = np_sub(X[2], c1.Ow[2]);
    const float g0 = np_sub(X[0], c2.Ow[0]), g1 = np_sub(X[1], c2.Ow[1]), g2 = np_sub(X[2], c2.Ow[2]);
    const float dist1 = np_sqrt(np_dot3(e0, e1, e2, e0, e1, e2)), dist2 = np_sqrt(np_dot3(g0, g1, g2, g0, g1, g2));
    if (dist1 == 0.0f || dist2 == 0.0f) return kNpZeroDist;
    if (th_far > 0.0f && (dist1 >= th_far || dist2 >= th_far)) return kNpFar;
    const float ratio_dist = np_div(dist2, dist1), ratio_octave = np_div(f1.scale, f2.scale);
    if (np_mul(ratio_dist, ratio_factor) < ratio_octave || ratio_dist > np_mul(ratio_octave, ratio_factor)) return kNpScaleRatio;
    return made;
}

}  // namespace msorb
