// TwoViewReconstruction (src/TwoViewReconstruction.cc) for a pinhole camera: ComputeH21 / ComputeF21 on eight normalised pairs, the
// two terms of one match of CheckHomography / CheckFundamental, the motion hypotheses of ReconstructH / ReconstructF (DecomposeE)
// and one match of CheckRT.  One statement of the arithmetic for the kernels of two_view.hip and for the host: float, every operation
// a single correctly rounded IEEE operation in the reference's statement order, sums left to right, nothing contracted (the np_*
// operators of new_points_device.h); double only where the reference's expression is double.  DESIGN.md section 15 tabulates what
// the reference leaves to Eigen and what is fixed here instead.
//
// The 9-column null vector is written for `stride` cooperating lanes that share one TvWork (the device: the 256 threads of a
// workgroup, the work in LDS; the host: lane 0 of 1), in the manner of mlpnp_device.h: TV_SYNC() separates a phase that writes the
// work from one that reads it, and everything outside the `for (k = lane; ...)` loops is computed by every lane on the same values.
#pragma once
#include "new_points_device.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define TV_SYNC() __syncthreads()
#else
#define TV_SYNC() ((void)0)
#endif

namespace msorb {

constexpr int kTvMaxSweeps = 30;    // one-sided Jacobi on 9 columns in float; the bound keeps a workgroup from spinning on garbage
constexpr int kTvMaxSweeps3 = 30;   // two-sided Jacobi on a 3x3

struct TvWork {
    float A[16][9];   // the design matrix (8 rows for F), rotated in place
    float V[9][9];
};

// ---- 3x3 helpers; matrices are row major

// C = A * B as Eigen's lazy product gives each coefficient: (a0 b0 + a1 b1) + a2 b2
NP_HD void tv_mul3(const float* A, const float* B, float* C) {
NP_UNROLL
    for (int r = 0; r < 3; r++)
NP_UNROLL
        for (int c = 0; c < 3; c++) C[3 * r + c] = np_dot3(A[3 * r], A[3 * r + 1], A[3 * r + 2], B[c], B[3 + c], B[6 + c]);
}
NP_HD void tv_transpose3(const float* A, float* T) {
NP_UNROLL
    for (int r = 0; r < 3; r++)
NP_UNROLL
        for (int c = 0; c < 3; c++) T[3 * r + c] = A[3 * c + r];
}
// m(0,a) * (m(1,b) m(2,c) - m(1,c) m(2,b))
NP_HD float tv_det3_term(const float* M, int a, int b, int c) { return np_mul(M[a], np_axmby(M[3 + b], M[6 + c], M[3 + c], M[6 + b])); }
// (term(0,1,2) - term(1,0,2)) + term(2,0,1)
NP_HD float tv_det3(const float* M) { return np_add(np_sub(tv_det3_term(M, 0, 1, 2), tv_det3_term(M, 1, 0, 2)), tv_det3_term(M, 2, 0, 1)); }
// adjugate / determinant: cofactor(i, j) = M(i+1, j+1) M(i+2, j+2) - M(i+1, j+2) M(i+2, j+1) (indices mod 3), the determinant the
// first row against its cofactors summed left to right, inv(j, i) = cofactor(i, j) * (1 / det)
NP_HD void tv_inverse3(const float* M, float* inv) {
    float cof[9];
NP_UNROLL
    for (int i = 0; i < 3; i++)
NP_UNROLL
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            cof[3 * i + j] = np_axmby(M[3 * i1 + j1], M[3 * i2 + j2], M[3 * i1 + j2], M[3 * i2 + j1]);
        }
    const float det = np_dot3(M[0], M[1], M[2], cof[0], cof[1], cof[2]);
    const float invdet = np_div(1.0f, det);
NP_UNROLL
    for (int i = 0; i < 3; i++)
NP_UNROLL
        for (int j = 0; j < 3; j++) inv[3 * j + i] = np_mul(cof[3 * i + j], invdet);
}

// Eigen::JacobiSVD<Matrix3f> with ComputeFullU | ComputeFullV, as far as that algorithm is publicly described: the two-sided Jacobi
// of np_null_vector (new_points_device.h) on a 3x3, U accumulated with the left rotations' transposes, then the diagonal made
// non-negative by negating U's column, the singular values scaled back and put in descending order by selection with swaps, U's and
// V's columns following.  A = U diag(S) V^T.
NP_HD void tv_svd3(const float* A, float* U, float* S, float* V) {
    const float tiny = 1.17549435e-38f, precision = 2.384185791015625e-07f;   // FLT_MIN, 2 * FLT_EPSILON
    float W[3][3], Um[3][3], Vm[3][3];
    float scale = 0.0f;
NP_UNROLL
    for (int i = 0; i < 9; i++) scale = np_max(scale, np_abs(A[i]));
    if (!(scale > 0.0f) || !(scale <= 3.402823466e+38f)) scale = 1.0f;   // zero, NaN or infinite
NP_UNROLL
    for (int i = 0; i < 3; i++)
NP_UNROLL
        for (int j = 0; j < 3; j++) { W[i][j] = np_div(A[3 * i + j], scale); Um[i][j] = Vm[i][j] = i == j ? 1.0f : 0.0f; }
    float max_diag = np_max(np_max(np_abs(W[0][0]), np_abs(W[1][1])), np_abs(W[2][2]));
    for (int sweep = 0; sweep < kTvMaxSweeps3; sweep++) {
        bool finished = true;
NP_UNROLL
        for (int p = 1; p < 3; p++)
NP_UNROLL
            for (int q = 0; q < p; q++) {
                const float thr = np_max(tiny, np_mul(precision, max_diag));
                if (!(np_abs(W[p][q]) > thr || np_abs(W[q][p]) > thr)) continue;
                finished = false;
                const float m00 = W[p][p], m01 = W[p][q], m10 = W[q][p], m11 = W[q][q];
                const float t = np_add(m00, m11), d = np_sub(m10, m01);
                float c1 = 1.0f, s1 = 0.0f;
                if (!(np_abs(d) < tiny)) {
                    const float u = np_div(t, d), tmp = np_sqrt(np_add(1.0f, np_mul(u, u)));
                    s1 = np_div(1.0f, tmp);
                    c1 = np_div(u, tmp);
                }
                const float n00 = np_axpby(c1, m00, s1, m10), n01 = np_axpby(c1, m01, s1, m11), n11 = np_axmby(c1, m11, s1, m01);
                float cr = 1.0f, sr = 0.0f;
                const float deno = np_mul(2.0f, np_abs(n01));
                if (!(deno < tiny)) {
                    const float tau = np_div(np_sub(n00, n11), deno), w = np_sqrt(np_add(np_mul(tau, tau), 1.0f));
                    const float tt = tau > 0.0f ? np_div(1.0f, np_add(tau, w)) : np_div(1.0f, np_sub(tau, w));
                    const float n = np_div(1.0f, np_sqrt(np_add(np_mul(tt, tt), 1.0f)));
                    const float mag = np_mul(np_abs(tt), n);
                    sr = ((tt > 0.0f) == (n01 > 0.0f)) ? -mag : mag;
                    cr = n;
                }
                const float cl = np_axpby(c1, cr, s1, sr), sl = np_axmby(s1, cr, c1, sr);
NP_UNROLL
                for (int k = 0; k < 3; k++) {   // W.applyOnTheLeft(p, q, j_left); U.applyOnTheRight(p, q, j_left.transpose())
                    const float a = W[p][k], b = W[q][k];
                    W[p][k] = np_axpby(cl, a, sl, b);
                    W[q][k] = np_axmby(cl, b, sl, a);
                    const float ua = Um[k][p], ub = Um[k][q];
                    Um[k][p] = np_axpby(cl, ua, sl, ub);
                    Um[k][q] = np_axmby(cl, ub, sl, ua);
                }
NP_UNROLL
                for (int k = 0; k < 3; k++) {   // W.applyOnTheRight(p, q, j_right); V.applyOnTheRight(p, q, j_right)
                    const float a = W[k][p], b = W[k][q];
                    W[k][p] = np_axmby(cr, a, sr, b);
                    W[k][q] = np_axpby(sr, a, cr, b);
                    const float va = Vm[k][p], vb = Vm[k][q];
                    Vm[k][p] = np_axmby(cr, va, sr, vb);
                    Vm[k][q] = np_axpby(sr, va, cr, vb);
                }
                max_diag = np_max(max_diag, np_max(np_abs(W[p][p]), np_abs(W[q][q])));
            }
        if (finished) break;
    }
    float sv[3];
NP_UNROLL
    for (int i = 0; i < 3; i++) {
        const float a = W[i][i];
        sv[i] = np_abs(a);
        if (a < 0.0f) {
NP_UNROLL
            for (int k = 0; k < 3; k++) Um[k][i] = -Um[k][i];
        }
    }
NP_UNROLL
    for (int i = 0; i < 3; i++) sv[i] = np_mul(sv[i], scale);
    // descending order by selection: position i takes the first maximum of positions i..2 (a swap of values and columns)
NP_UNROLL
    for (int i = 0; i < 2; i++) {
        float best = sv[i];
        int pos = i;
NP_UNROLL
        for (int k = i + 1; k < 3; k++)
            if (sv[k] > best) { best = sv[k]; pos = k; }
NP_UNROLL
        for (int k = i + 1; k < 3; k++)
            if (k == pos) {
                const float ts = sv[i]; sv[i] = sv[k]; sv[k] = ts;
NP_UNROLL
                for (int r = 0; r < 3; r++) {
                    const float tu = Um[r][i]; Um[r][i] = Um[r][k]; Um[r][k] = tu;
                    const float tv = Vm[r][i]; Vm[r][i] = Vm[r][k]; Vm[r][k] = tv;
                }
            }
    }
NP_UNROLL
    for (int i = 0; i < 3; i++) {
        S[i] = sv[i];
NP_UNROLL
        for (int j = 0; j < 3; j++) { U[3 * i + j] = Um[i][j]; V[3 * i + j] = Vm[i][j]; }
    }
}

// ---- the null vector of the design matrix (:267-269, :298-300 take V.col(8) of Eigen::JacobiSVD<MatrixXf>)

// One-sided (Hestenes) Jacobi on the 9 columns of w.A (rows x 9, filled and synchronised by the caller), in float, never forming
// A^T A.  The pairs (p, q), p = 0..7, q = p+1..8 in that cyclic order; for a pair, alpha = |a_p|^2, beta = |a_q|^2, gamma = a_p . a_q
// summed over the rows in ascending order; the pair is rotated when |gamma| > max(FLT_MIN, 2 eps sqrt(alpha beta)) and both alpha and
// beta exceed (16 eps)^2 times the largest column norm the matrix started with (a column below that is the null column at its
// rounding floor: against it gamma is noise, and rotating it again would never end), with
//   tau = (beta - alpha) / (2 gamma),  t = 1 / (tau +- sqrt(tau^2 + 1)) (the sign of tau),  c = 1 / sqrt(t^2 + 1),  s = t c,
//   a_p <- c a_p - s a_q,  a_q <- s a_p + c a_q,  the same on V's columns.
// Sweeps until one passes without a rotation or kTvMaxSweeps are done.  x = the column of V whose column of A has the smallest norm
// (the first minimum).  The sign of x is whatever the rotations leave.  Every lane returns the same x; w may be reused after the
// closing TV_SYNC.
//
// Non-finite input: a column that holds a NaN is never rotated (its alpha, and every gamma against it, fails the comparisons; np_max
// keeps it out of max_norm); the other columns rotate among themselves as usual and x comes from them, finite, unless the NaN is in
// column 0, whose NaN norm no later one compares below: then x is the first unit vector.  One infinity makes max_norm and the floor
// infinite: nothing rotates and x is the unit vector of the first smallest column (the first unit vector for an all-infinite A).
// A NaN in A therefore does not show as a NaN in x.
//
// Domain.  With N the largest column norm of A at entry, the rotation test is the relative one stated above while
// 2^-12 <= N <= 2^30: alpha beta is formed in float, every column the floor admits has alpha > 2^-38 N^2, so alpha beta > 2^-76 N^4
// >= FLT_MIN, and no column outgrows the Frobenius norm <= 3 N, so alpha beta <= 81 N^4 < FLT_MAX.  The callers are inside it:
// Normalize leaves mean deviation 1 per coordinate, so the column of ones has norm sqrt(8) and a coordinate is at most n / 2 for n
// matches (mean deviation >= 2 |x_i - mean| / n), n <= 32 768: entries up to 2^28, N <= 2^29.5.  Outside (tests/decomp_cases.py
// walks it): down to N ~ 2^-31 and up to 2^31 random matrices still give the same bits scaled; from 2^-36 to 2^-54 alpha beta
// underflows, the threshold is FLT_MIN alone, rounding noise keeps rotating and the sweeps run to kTvMaxSweeps, x still accurate;
// below 2^-56 x loses accuracy; below 2^-62 (gamma < FLT_MIN) and above 2^33 (alpha beta overflows, the threshold is infinite)
// nothing rotates and x is the unit vector of the first smallest column of A as given.
NP_HD void tv_null_vector(TvWork& w, int lane, int stride, int rows, float* x) {
    const float tiny = 1.17549435e-38f, precision = 2.384185791015625e-07f;   // FLT_MIN, 2 * FLT_EPSILON
    const float floor_rel = 3.63797880709171295e-12f;                          // (16 * FLT_EPSILON)^2 = 2^-38
    for (int k = lane; k < 81; k += stride) w.V[k / 9][k % 9] = k / 9 == k % 9 ? 1.0f : 0.0f;
    float max_norm = 0.0f;
    for (int c = 0; c < 9; c++) {
        float s = np_mul(w.A[0][c], w.A[0][c]);
        for (int k = 1; k < rows; k++) s = np_add(s, np_mul(w.A[k][c], w.A[k][c]));
        max_norm = np_max(max_norm, s);
    }
    const float floor2 = np_mul(floor_rel, max_norm);
    TV_SYNC();
    for (int sweep = 0; sweep < kTvMaxSweeps; sweep++) {
        bool finished = true;
        for (int p = 0; p < 8; p++)
            for (int q = p + 1; q < 9; q++) {
                float alpha = np_mul(w.A[0][p], w.A[0][p]), beta = np_mul(w.A[0][q], w.A[0][q]), gamma = np_mul(w.A[0][p], w.A[0][q]);
                for (int k = 1; k < rows; k++) {
                    const float a = w.A[k][p], b = w.A[k][q];
                    alpha = np_add(alpha, np_mul(a, a));
                    beta = np_add(beta, np_mul(b, b));
                    gamma = np_add(gamma, np_mul(a, b));
                }
                const float thr = np_max(tiny, np_mul(precision, np_sqrt(np_mul(alpha, beta))));
                if (!(np_abs(gamma) > thr) || !(alpha > floor2) || !(beta > floor2)) continue;   // the same on every lane
                finished = false;
                const float tau = np_div(np_sub(beta, alpha), np_mul(2.0f, gamma));
                const float ww = np_sqrt(np_add(np_mul(tau, tau), 1.0f));
                const float t = tau >= 0.0f ? np_div(1.0f, np_add(tau, ww)) : np_div(1.0f, np_sub(tau, ww));
                const float c = np_div(1.0f, np_sqrt(np_add(np_mul(t, t), 1.0f)));
                const float s = np_mul(t, c);
                TV_SYNC();   // every lane has read the two columns
                for (int k = lane; k < rows + 9; k += stride) {
                    float* row = k < rows ? w.A[k] : w.V[k - rows];
                    const float a = row[p], b = row[q];
                    row[p] = np_axmby(c, a, s, b);
                    row[q] = np_axpby(s, a, c, b);
                }
                TV_SYNC();
            }
        if (finished) break;
    }
    int best = 0;
    float least = 0.0f;
    for (int c = 0; c < 9; c++) {
        float s = np_mul(w.A[0][c], w.A[0][c]);
        for (int k = 1; k < rows; k++) s = np_add(s, np_mul(w.A[k][c], w.A[k][c]));
        if (c == 0 || s < least) { least = s; best = c; }
    }
NP_UNROLL
    for (int i = 0; i < 9; i++) x[i] = w.V[i][best];
    TV_SYNC();
}

// :238-265 the rows 2 i, 2 i + 1 of ComputeH21's A from pair i (pn: u1, v1, u2, v2 normalised)
NP_HD void tv_fill_h_rows(TvWork& w, int i, const float* pn) {
    const float u1 = pn[0], v1 = pn[1], u2 = pn[2], v2 = pn[3];
    float* a = w.A[2 * i];
    float* b = w.A[2 * i + 1];
    a[0] = 0.0f; a[1] = 0.0f; a[2] = 0.0f; a[3] = -u1; a[4] = -v1; a[5] = -1.0f;
    a[6] = np_mul(v2, u1); a[7] = np_mul(v2, v1); a[8] = v2;
    b[0] = u1; b[1] = v1; b[2] = 1.0f; b[3] = 0.0f; b[4] = 0.0f; b[5] = 0.0f;
    b[6] = np_mul(-u2, u1); b[7] = np_mul(-u2, v1); b[8] = -u2;
}
// :280-296 row i of ComputeF21's A
NP_HD void tv_fill_f_row(TvWork& w, int i, const float* pn) {
    const float u1 = pn[0], v1 = pn[1], u2 = pn[2], v2 = pn[3];
    float* a = w.A[i];
    a[0] = np_mul(u2, u1); a[1] = np_mul(u2, v1); a[2] = u2;
    a[3] = np_mul(v2, u1); a[4] = np_mul(v2, v1); a[5] = v2;
    a[6] = u1; a[7] = v1; a[8] = 1.0f;
}

// Normalize's T (:778-783) from mean and scale: [sX 0 -meanX sX; 0 sY -meanY sY; 0 0 1]
struct TvNorm { float mean_x, mean_y, sx, sy; };
NP_HD void tv_norm_matrix(const TvNorm& n, float* T) {
    T[0] = n.sx; T[1] = 0.0f; T[2] = np_mul(-n.mean_x, n.sx);
    T[3] = 0.0f; T[4] = n.sy; T[5] = np_mul(-n.mean_y, n.sy);
    T[6] = 0.0f; T[7] = 0.0f; T[8] = 1.0f;
}
// :759-760, :774-775 one keypoint
NP_HD void tv_normalize_point(const TvNorm& n, float x, float y, float& xn, float& yn) {
    xn = np_mul(np_sub(x, n.mean_x), n.sx);
    yn = np_mul(np_sub(y, n.mean_y), n.sy);
}

// :166-168 from the null vector x: H21i = (T2inv * Hn) * T1 with T2inv = tv_inverse3(T2), H12i = tv_inverse3(H21i)
NP_HD void tv_homography_from_null(const float* x, const float* T1, const float* T2, float* H21, float* H12) {
    float T2inv[9], tmp[9];
    tv_inverse3(T2, T2inv);
    tv_mul3(T2inv, x, tmp);
    tv_mul3(tmp, T1, H21);
    tv_inverse3(H21, H12);
}
// :300-307, :219 from the null vector x: the rank-2 step (U * diag(w0, w1, 0)) * V^T, then F21i = (T2^T * Fn) * T1
NP_HD void tv_fundamental_from_null(const float* x, const float* T1, const float* T2, float* F21) {
    float U[9], S[3], V[9], UD[9], Vt[9], Fn[9], T2t[9], tmp[9];
    tv_svd3(x, U, S, V);
    S[2] = 0.0f;
NP_UNROLL
    for (int i = 0; i < 3; i++)
NP_UNROLL
        for (int j = 0; j < 3; j++) UD[3 * i + j] = np_mul(U[3 * i + j], S[j]);
    tv_transpose3(V, Vt);
    tv_mul3(UD, Vt, Fn);
    tv_transpose3(T2, T2t);
    tv_mul3(T2t, Fn, tmp);
    tv_mul3(tmp, T1, F21);
}

// const float invSigmaSquare = 1.0 / (sigma * sigma) (:340, :416)
NP_HD float tv_inv_sigma_square(float sigma) { return (float)np_ddiv(1.0, (double)np_mul(sigma, sigma)); }

// One i of CheckHomography (:342-390).  t1, t2: what the match adds to the score, in that order; a rejected term is +0.0f, which
// adds exactly; a NaN chi-square is not > th and is added as the reference adds it.  Returns bIn.
NP_HD bool tv_homography_terms(const float* H21, const float* H12, float u1, float v1, float u2, float v2, float inv_sigma_square,
                               float& t1, float& t2) {
    const float th = 5.991f;
    bool in = true;
    const float w2in1inv = (float)np_ddiv(1.0, (double)np_add(np_axpby(H12[6], u2, H12[7], v2), H12[8]));
    const float u2in1 = np_mul(np_add(np_axpby(H12[0], u2, H12[1], v2), H12[2]), w2in1inv);
    const float v2in1 = np_mul(np_add(np_axpby(H12[3], u2, H12[4], v2), H12[5]), w2in1inv);
    const float dx1 = np_sub(u1, u2in1), dy1 = np_sub(v1, v2in1);
    const float chi1 = np_mul(np_add(np_mul(dx1, dx1), np_mul(dy1, dy1)), inv_sigma_square);
    if (chi1 > th) { in = false; t1 = 0.0f; } else t1 = np_sub(th, chi1);
    const float w1in2inv = (float)np_ddiv(1.0, (double)np_add(np_axpby(H21[6], u1, H21[7], v1), H21[8]));
    const float u1in2 = np_mul(np_add(np_axpby(H21[0], u1, H21[1], v1), H21[2]), w1in2inv);
    const float v1in2 = np_mul(np_add(np_axpby(H21[3], u1, H21[4], v1), H21[5]), w1in2inv);
    const float dx2 = np_sub(u2, u1in2), dy2 = np_sub(v2, v1in2);
    const float chi2 = np_mul(np_add(np_mul(dx2, dx2), np_mul(dy2, dy2)), inv_sigma_square);
    if (chi2 > th) { in = false; t2 = 0.0f; } else t2 = np_sub(th, chi2);
    return in;
}

// One i of CheckFundamental (:418-470)
NP_HD bool tv_fundamental_terms(const float* F, float u1, float v1, float u2, float v2, float inv_sigma_square, float& t1, float& t2) {
    const float th = 3.841f, th_score = 5.991f;
    bool in = true;
    const float a2 = np_add(np_axpby(F[0], u1, F[1], v1), F[2]);
    const float b2 = np_add(np_axpby(F[3], u1, F[4], v1), F[5]);
    const float c2 = np_add(np_axpby(F[6], u1, F[7], v1), F[8]);
    const float num2 = np_add(np_axpby(a2, u2, b2, v2), c2);
    const float chi1 = np_mul(np_div(np_mul(num2, num2), np_add(np_mul(a2, a2), np_mul(b2, b2))), inv_sigma_square);
    if (chi1 > th) { in = false; t1 = 0.0f; } else t1 = np_sub(th_score, chi1);
    const float a1 = np_add(np_axpby(F[0], u2, F[3], v2), F[6]);
    const float b1 = np_add(np_axpby(F[1], u2, F[4], v2), F[7]);
    const float c1 = np_add(np_axpby(F[2], u2, F[5], v2), F[8]);
    const float num1 = np_add(np_axpby(a1, u1, b1, v1), c1);
    const float chi2 = np_mul(np_div(np_mul(num1, num1), np_add(np_mul(a1, a1), np_mul(b1, b1))), inv_sigma_square);
    if (chi2 > th) { in = false; t2 = 0.0f; } else t2 = np_sub(th_score, chi2);
    return in;
}

// ---- motion hypotheses

NP_HD void tv_k_matrix(const float* cam, float* K) {   // Pinhole::toK_: fx, fy, cx, cy, no skew
    K[0] = cam[0]; K[1] = 0.0f; K[2] = cam[2];
    K[3] = 0.0f; K[4] = cam[1]; K[5] = cam[3];
    K[6] = 0.0f; K[7] = 0.0f; K[8] = 1.0f;
}

NP_HD void tv_normalize3(const float* v, float* out) {   // v / v.norm()
    const float n = np_sqrt(np_dot3(v[0], v[1], v[2], v[0], v[1], v[2]));
NP_UNROLL
    for (int i = 0; i < 3; i++) out[i] = np_div(v[i], n);
}

// ReconstructF's four hypotheses (:484-503, DecomposeE :903-927): E21 = (K^T * F21) * K; R[4][9], t[4][3] in the order
// (R1, t) (R2, t) (R1, -t) (R2, -t).
NP_HD void tv_motions_from_f(const float* F21, const float* cam, float* R, float* t) {
    float K[9], Kt[9], tmp[9], E[9], U[9], S[3], V[9], Vt[9], R1[9], R2[9], tt[3];
    tv_k_matrix(cam, K);
    tv_transpose3(K, Kt);
    tv_mul3(Kt, F21, tmp);
    tv_mul3(tmp, K, E);
    tv_svd3(E, U, S, V);
    tv_transpose3(V, Vt);
    const float u2[3] = {U[2], U[5], U[8]};
    tv_normalize3(u2, tt);
    const float W[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float Wt[9];
    tv_transpose3(W, Wt);
    tv_mul3(U, W, tmp);
    tv_mul3(tmp, Vt, R1);
    if (tv_det3(R1) < 0.0f) {
NP_UNROLL
        for (int k = 0; k < 9; k++) R1[k] = -R1[k];
    }
    tv_mul3(U, Wt, tmp);
    tv_mul3(tmp, Vt, R2);
    if (tv_det3(R2) < 0.0f) {
NP_UNROLL
        for (int k = 0; k < 9; k++) R2[k] = -R2[k];
    }
NP_UNROLL
    for (int k = 0; k < 9; k++) { R[k] = R1[k]; R[9 + k] = R2[k]; R[18 + k] = R1[k]; R[27 + k] = R2[k]; }
NP_UNROLL
    for (int k = 0; k < 3; k++) { t[k] = tt[k]; t[3 + k] = tt[k]; t[6 + k] = -tt[k]; t[9 + k] = -tt[k]; }
}

// ReconstructH's eight hypotheses (:582-690); false: the return of :597-600.  The normals (vn) are never read and are not formed.
NP_HD bool tv_motions_from_h(const float* H21, const float* cam, float* R, float* t) {
    float K[9], invK[9], tmp[9], A[9], U[9], w[3], V[9], Vt[9];
    tv_k_matrix(cam, K);
    tv_inverse3(K, invK);
    tv_mul3(invK, H21, tmp);
    tv_mul3(tmp, K, A);
    tv_svd3(A, U, w, V);
    tv_transpose3(V, Vt);
    const float s = np_mul(tv_det3(U), tv_det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)np_div(d1, d2) < 1.00001 || (double)np_div(d2, d3) < 1.00001) return false;
    const float d11 = np_mul(d1, d1), d22 = np_mul(d2, d2), d33 = np_mul(d3, d3);
    const float aux1 = np_sqrt(np_div(np_sub(d11, d22), np_sub(d11, d33)));
    const float aux3 = np_sqrt(np_div(np_sub(d22, d33), np_sub(d11, d33)));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float root = np_sqrt(np_mul(np_sub(d11, d22), np_sub(d22, d33)));
    const float aux_stheta = np_div(root, np_mul(np_add(d1, d3), d2));
    const float ctheta = np_div(np_add(d22, np_mul(d1, d3)), np_mul(np_add(d1, d3), d2));
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = np_div(root, np_mul(np_sub(d1, d3), d2));
    const float cphi = np_div(np_sub(np_mul(d1, d3), d22), np_mul(np_sub(d1, d3), d2));
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    float sU[9];
NP_UNROLL
    for (int k = 0; k < 9; k++) sU[k] = np_mul(s, U[k]);
NP_UNROLL
    for (int i = 0; i < 8; i++) {
        const int j = i & 3;
        float Rp[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float tp[3];
        if (i < 4) {   // d' = d2
            Rp[0] = ctheta; Rp[2] = -stheta[j]; Rp[4] = 1.0f; Rp[6] = stheta[j]; Rp[8] = ctheta;
            const float f = np_sub(d1, d3);
            tp[0] = np_mul(x1[j], f); tp[1] = np_mul(0.0f, f); tp[2] = np_mul(-x3[j], f);
        } else {       // d' = -d2
            Rp[0] = cphi; Rp[2] = sphi[j]; Rp[4] = -1.0f; Rp[6] = sphi[j]; Rp[8] = -cphi;
            const float f = np_add(d1, d3);
            tp[0] = np_mul(x1[j], f); tp[1] = np_mul(0.0f, f); tp[2] = np_mul(x3[j], f);
        }
        tv_mul3(sU, Rp, tmp);
        tv_mul3(tmp, Vt, R + 9 * i);
        float tu[3];
NP_UNROLL
        for (int r = 0; r < 3; r++) tu[r] = np_dot3(U[3 * r], U[3 * r + 1], U[3 * r + 2], tp[0], tp[1], tp[2]);
        tv_normalize3(tu, t + 3 * i);
    }
    return true;
}

// ---- CheckRT (:786-901)

struct TvPose {       // what CheckRT sets up before its loop
    float P1[12], P2[12];   // K [I | 0], K [R | t], 3x4 row major
    float R[9], t[3], O2[3];
    float fx, fy, cx, cy;
    float th2;              // 4.0 * mSigma2 narrowed to the float parameter
};

NP_HD void tv_pose_setup(const float* R, const float* t, const float* cam, float sigma, TvPose& P) {
    float K[9];
    tv_k_matrix(cam, K);
NP_UNROLL
    for (int r = 0; r < 3; r++) {
NP_UNROLL
        for (int c = 0; c < 3; c++) {
            P.P1[4 * r + c] = K[3 * r + c];
            P.P2[4 * r + c] = np_dot3(K[3 * r], K[3 * r + 1], K[3 * r + 2], R[c], R[3 + c], R[6 + c]);
        }
        P.P1[4 * r + 3] = 0.0f;
        P.P2[4 * r + 3] = np_dot3(K[3 * r], K[3 * r + 1], K[3 * r + 2], t[0], t[1], t[2]);
    }
NP_UNROLL
    for (int k = 0; k < 9; k++) P.R[k] = R[k];
NP_UNROLL
    for (int k = 0; k < 3; k++) {
        P.t[k] = t[k];
        P.O2[k] = -np_dot3(R[k], R[3 + k], R[6 + k], t[0], t[1], t[2]);   // -R^T * t: negating the factors or the sum gives the same bits
    }
    P.fx = cam[0]; P.fy = cam[1]; P.cx = cam[2]; P.cy = cam[3];
    P.th2 = (float)np_dmul(4.0, (double)np_mul(sigma, sigma));
}

enum TvPoint : int { kTvRejected = 0, kTvCounted = 1, kTvGood = 2 };   // not in nGood / in nGood / in nGood and vbGood

// One inlier match of CheckRT's loop (:825-887).  kTvCounted and kTvGood write X (vP3D) and cos_parallax (pushed to vCosParallax).
// GeometricTools::Triangulate is the statement of new_points_device.h (np_null_vector on the four rows of GeometricTools.cc:50-53);
// CheckRT ignores its return value and reads an unassigned vector when x3Dh(3) == 0: here such a match is not finite (:835).
NP_HD int tv_check_point(const TvPose& P, float u1, float v1, float u2, float v2, float* X, float& cos_parallax) {
    float A[16], xh[4];
NP_UNROLL
    for (int k = 0; k < 4; k++) {
        A[k] = np_sub(np_mul(u1, P.P1[8 + k]), P.P1[k]);
        A[4 + k] = np_sub(np_mul(v1, P.P1[8 + k]), P.P1[4 + k]);
        A[8 + k] = np_sub(np_mul(u2, P.P2[8 + k]), P.P2[k]);
        A[12 + k] = np_sub(np_mul(v2, P.P2[8 + k]), P.P2[4 + k]);
    }
    np_null_vector(A, xh);
    if (xh[3] == 0.0f) return kTvRejected;
    float p[3];
NP_UNROLL
    for (int i = 0; i < 3; i++) p[i] = np_div(xh[i], xh[3]);
    const float big = 3.402823466e+38f;
    if (!(np_abs(p[0]) <= big) || !(np_abs(p[1]) <= big) || !(np_abs(p[2]) <= big)) return kTvRejected;   // !isfinite
    const float dist1 = np_sqrt(np_dot3(p[0], p[1], p[2], p[0], p[1], p[2]));
    const float n2[3] = {np_sub(p[0], P.O2[0]), np_sub(p[1], P.O2[1]), np_sub(p[2], P.O2[2])};
    const float dist2 = np_sqrt(np_dot3(n2[0], n2[1], n2[2], n2[0], n2[1], n2[2]));
    const float cosp = np_div(np_dot3(p[0], p[1], p[2], n2[0], n2[1], n2[2]), np_mul(dist1, dist2));
    const bool low = (double)cosp < 0.99998;
    if (p[2] <= 0.0f && low) return kTvRejected;
    float p2[3];
NP_UNROLL
    for (int r = 0; r < 3; r++) p2[r] = np_add(np_dot3(P.R[3 * r], P.R[3 * r + 1], P.R[3 * r + 2], p[0], p[1], p[2]), P.t[r]);
    if (p2[2] <= 0.0f && low) return kTvRejected;
    const float invz1 = (float)np_ddiv(1.0, (double)p[2]);
    const float ex1 = np_sub(np_add(np_mul(np_mul(P.fx, p[0]), invz1), P.cx), u1);
    const float ey1 = np_sub(np_add(np_mul(np_mul(P.fy, p[1]), invz1), P.cy), v1);
    if (np_add(np_mul(ex1, ex1), np_mul(ey1, ey1)) > P.th2) return kTvRejected;
    const float invz2 = (float)np_ddiv(1.0, (double)p2[2]);
    const float ex2 = np_sub(np_add(np_mul(np_mul(P.fx, p2[0]), invz2), P.cx), u2);
    const float ey2 = np_sub(np_add(np_mul(np_mul(P.fy, p2[1]), invz2), P.cy), v2);
    if (np_add(np_mul(ex2, ex2), np_mul(ey2, ey2)) > P.th2) return kTvRejected;
    X[0] = p[0]; X[1] = p[1]; X[2] = p[2];
    cos_parallax = cosp;
    return low ? kTvGood : kTvCounted;
}

}  // namespace msorb
