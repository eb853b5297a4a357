// MLPnPsolver::computePose for exactly six correspondences (src/MLPnPsolver.cpp:399-701, with rot2rodrigues :720-735, rodrigues2rot
// :703-718, mlpnp_gn :737-801 and mlpnp_residuals_and_jacs :803-849) and one correspondence of MLPnPsolver::CheckInliers (:305-336)
// for a pinhole camera.  One statement of the arithmetic for the device (mlpnp_hypotheses_kernel, mlpnp.hip) and the host
// (tests/mlpnp_main.cc, tools/mlpnp_ransac_host.cc): double, every operation a single correctly rounded IEEE operation (the np_d*
// operators of new_points_device.h), sums taken left to right in ascending index unless a comment says otherwise, nothing contracted.
// sin, cos, acos, pow and sqrt are the platform's.
//
// The work is written for `stride` cooperating lanes that share one MlpnpWork (the device: the 64 lanes of a wavefront, the work in
// LDS; the host: lane 0 of 1): a loop `for (k = lane; k < n; k += stride)` gives item k to one lane, MLPNP_SYNC() separates a phase
// that writes the work from one that reads it, and everything outside such loops is computed by every lane on the same values.  No
// item of a phase reads what another item of that phase writes, so the host's serial order and the device's lanes give the same
// bits.
//
// What the reference leaves to Eigen is fixed here instead:
//   nullspace of a bearing f (:414-416, the last two right singular vectors of f^T): with n = f / |f| and s = the sign of n.z,
//       a = -1 / (s + n.z), b = n.x n.y a:   column 0 = (1 + s n.x^2 a, s b, -s n.x),  column 1 = (b, s + n.y^2 a, -n.y).
//       Any orthonormal basis of that plane gives the same A^T A, J^T J and J^T r; only the |J dx| < 1e-5 stop test sees the basis.
//   rank of P P^T (:424-432, FullPivHouseholderQR<Matrix3d>::rank()): Householder QR with full pivoting, the pivot of step k the
//       first largest |entry| of the remaining corner in column-major order, the decomposition ending early when that entry is
//       <= 3 eps times the first pivot's, rank = the number of |R(i,i)| > 3 eps max|R(i,i)| (the default threshold rule).
//   eigenvectors of the symmetric 3x3 P P^T (:437-438): cyclic Jacobi, eigenvalues in increasing order (stable), row k of
//       eigenRot = eigenvector k; the signs are what the rotations leave.
//   right singular vector of A^T A's smallest singular value (:566-567, JacobiSVD of a 12x12 or 9x9): cyclic Jacobi on the symmetric
//       matrix, the pairs (p, q), p < q, in lexicographic order, a pair rotated when |W(p,q)| > max(DBL_MIN, 2 eps max|W(i,i)|),
//       sweeps until one passes without a rotation or kMlpnpMaxSweeps are done; the column of the first smallest |W(i,i)|.  Its
//       sign does not reach the result.
//   U V^T of the 3x3 SVD (:589-590, :648-649): one-sided Jacobi on the columns, pairs (0,1) (0,2) (1,2), a pair rotated when
//       |g_i . g_j| > max(DBL_MIN, 2 eps sqrt(|g_i|^2 |g_j|^2)); U = the columns divided by their norms.  A zero column gives a
//       non-finite rotation.
//   inverse of [R | t] (:667): [R^T | -(R^T t)].
//   the 6x6 solve (:783-784, LDLT): L D L^T without pivoting.
//   the Jacobian (:851-1000 is generated text and is not restated): the chain rule through the normalisation and the Rodrigues
//       map, mlpnp_residual_and_jacobian below.  It divides w by |w|, so it is non-finite at w = 0 as the reference's expression is
//       (0 * inf): such a hypothesis becomes NaN and counts no inlier.
#pragma once
#include "new_points_device.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define MLPNP_SYNC() __syncthreads()
#else
#define MLPNP_SYNC() ((void)0)
#endif

namespace msorb {

constexpr int kMlpnpMaxSweeps = 30;
constexpr double kMlpnpEps = 2.220446049250313e-16, kMlpnpTiny = 2.2250738585072014e-308;   // DBL_EPSILON, DBL_MIN

// hyp_flags_out: bit 0 planar, bits 1-3 the Gauss-Newton updates applied to x (0-5), bit 4 the loop was left by the break of :787
constexpr unsigned kMlpnpPlanar = 1u, kMlpnpBroke = 16u;

struct MlpnpWork {
    double f[6][3], p[6][3], q[6][3];   // bearings, world points (points3v), points3 (in the eigen frame when planar)
    double ns[6][2][3];                 // ns[i][c] = column c of nullspaces[i]
    double A[12][12], W[12][12], V[12][12];
    double J[12][6], r[12], S[6][6], g[6];
};

NP_HD double mp_dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
    return np_dadd(np_dadd(np_dmul(a0, b0), np_dmul(a1, b1)), np_dmul(a2, b2));
}
NP_HD double mp_norm3(const double* v) { return sqrt(mp_dot3(v[0], v[1], v[2], v[0], v[1], v[2])); }
NP_HD void mp_cross(const double* a, const double* b, double* c) {
    c[0] = np_dsub(np_dmul(a[1], b[2]), np_dmul(a[2], b[1]));
    c[1] = np_dsub(np_dmul(a[2], b[0]), np_dmul(a[0], b[2]));
    c[2] = np_dsub(np_dmul(a[0], b[1]), np_dmul(a[1], b[0]));
}
// y = M x (+ t), M row major
NP_HD void mp_mul3(const double* M, const double* x, double* y) {
    for (int r = 0; r < 3; r++) y[r] = mp_dot3(M[3 * r], M[3 * r + 1], M[3 * r + 2], x[0], x[1], x[2]);
}
NP_HD double mp_det3(const double* M) {
    const double c0 = np_dsub(np_dmul(M[4], M[8]), np_dmul(M[5], M[7]));
    const double c1 = np_dsub(np_dmul(M[3], M[8]), np_dmul(M[5], M[6]));
    const double c2 = np_dsub(np_dmul(M[3], M[7]), np_dmul(M[4], M[6]));
    return np_dadd(np_dsub(np_dmul(M[0], c0), np_dmul(M[1], c1)), np_dmul(M[2], c2));
}

// the c, s, t of the Jacobi rotation that zeroes the off-diagonal apq of [app apq; apq aqq]
NP_HD void mp_jacobi(double app, double aqq, double apq, double& c, double& s, double& t) {
    const double tau = np_ddiv(np_dsub(aqq, app), np_dmul(2.0, apq));
    const double w = sqrt(np_dadd(np_dmul(tau, tau), 1.0));
    t = tau >= 0.0 ? np_ddiv(1.0, np_dadd(tau, w)) : np_ddiv(1.0, np_dsub(tau, w));
    c = np_ddiv(1.0, sqrt(np_dadd(np_dmul(t, t), 1.0)));
    s = np_dmul(t, c);
}

NP_HD int mlpnp_rank3(const double* M) {
    const double prec = np_dmul(kMlpnpEps, 3.0);
    double a[3][3], piv[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 9; i++) a[i / 3][i % 3] = M[i];
    double biggest = 0.0, maxpivot = 0.0;
    int nonzero = 3;
    for (int k = 0; k < 3; k++) {
        double big = fabs(a[k][k]);
        int pr = k, pc = k;
        for (int c = k; c < 3; c++)
            for (int r = k; r < 3; r++)
                if (fabs(a[r][c]) > big) { big = fabs(a[r][c]); pr = r; pc = c; }
        if (k == 0) biggest = big;
        if (big <= np_dmul(biggest, prec)) { nonzero = k; break; }
        for (int j = 0; j < 3; j++) { const double x = a[k][j]; a[k][j] = a[pr][j]; a[pr][j] = x; }
        for (int i = 0; i < 3; i++) { const double x = a[i][k]; a[i][k] = a[i][pc]; a[i][pc] = x; }
        const double c0 = a[k][k];
        double tailsq = 0.0, ess[3] = {0.0, 0.0, 0.0}, tau = 0.0, beta = c0;
        for (int i = k + 1; i < 3; i++) tailsq = i == k + 1 ? np_dmul(a[i][k], a[i][k]) : np_dadd(tailsq, np_dmul(a[i][k], a[i][k]));
        if (!(tailsq <= kMlpnpTiny)) {
            beta = sqrt(np_dadd(np_dmul(c0, c0), tailsq));
            if (c0 >= 0.0) beta = -beta;
            for (int i = k + 1; i < 3; i++) ess[i] = np_ddiv(a[i][k], np_dsub(c0, beta));
            tau = np_ddiv(np_dsub(beta, c0), beta);
        }
        piv[k] = beta;
        if (fabs(beta) > maxpivot) maxpivot = fabs(beta);
        for (int j = k + 1; j < 3; j++) {
            double tmp = 0.0;
            for (int i = k + 1; i < 3; i++) tmp = i == k + 1 ? np_dmul(ess[i], a[i][j]) : np_dadd(tmp, np_dmul(ess[i], a[i][j]));
            tmp = np_dadd(tmp, a[k][j]);
            a[k][j] = np_dsub(a[k][j], np_dmul(tau, tmp));
            for (int i = k + 1; i < 3; i++) a[i][j] = np_dsub(a[i][j], np_dmul(np_dmul(tau, ess[i]), tmp));
        }
    }
    int rank = 0;
    for (int i = 0; i < nonzero; i++) rank += fabs(piv[i]) > np_dmul(maxpivot, prec);
    return rank;
}

// E (row major): row k = the eigenvector of the symmetric M's k-th smallest eigenvalue
NP_HD void mlpnp_eig3(const double* M, double* E) {
    double W[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { W[i][j] = M[3 * i + j]; V[i][j] = i == j ? 1.0 : 0.0; }
    double max_diag = fabs(W[0][0]);
    for (int i = 1; i < 3; i++) if (fabs(W[i][i]) > max_diag) max_diag = fabs(W[i][i]);
    for (int sweep = 0; sweep < kMlpnpMaxSweeps; sweep++) {
        bool finished = true;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                const double apq = W[p][q], thr = np_dmul(np_dmul(2.0, kMlpnpEps), max_diag);
                if (!(fabs(apq) > (thr > kMlpnpTiny ? thr : kMlpnpTiny))) continue;
                finished = false;
                const double app = W[p][p], aqq = W[q][q];
                double c, s, t;
                mp_jacobi(app, aqq, apq, c, s, t);
                for (int k = 0; k < 3; k++) {
                    if (k != p && k != q) {
                        const double akp = W[k][p], akq = W[k][q];
                        const double nkp = np_dsub(np_dmul(c, akp), np_dmul(s, akq)), nkq = np_dadd(np_dmul(s, akp), np_dmul(c, akq));
                        W[k][p] = nkp; W[p][k] = nkp; W[k][q] = nkq; W[q][k] = nkq;
                    }
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = np_dsub(np_dmul(c, vkp), np_dmul(s, vkq));
                    V[k][q] = np_dadd(np_dmul(s, vkp), np_dmul(c, vkq));
                }
                W[p][p] = np_dsub(app, np_dmul(t, apq));
                W[q][q] = np_dadd(aqq, np_dmul(t, apq));
                W[p][q] = 0.0; W[q][p] = 0.0;
                if (fabs(W[p][p]) > max_diag) max_diag = fabs(W[p][p]);
                if (fabs(W[q][q]) > max_diag) max_diag = fabs(W[q][q]);
            }
        if (finished) break;
    }
    bool used[3] = {false, false, false};
    for (int k = 0; k < 3; k++) {
        int best = -1;
        for (int i = 0; i < 3; i++)
            if (!used[i] && (best < 0 || W[i][i] < W[best][best])) best = i;
        used[best] = true;
        for (int r = 0; r < 3; r++) E[3 * k + r] = V[r][best];
    }
}

// U V^T of T = U S V^T (row major in and out)
NP_HD void mlpnp_nearest_rotation(const double* T, double* Rn) {
    double G[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { G[i][j] = T[3 * i + j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < kMlpnpMaxSweeps; sweep++) {
        bool finished = true;
        for (int i = 0; i < 2; i++)
            for (int j = i + 1; j < 3; j++) {
                const double alpha = mp_dot3(G[0][i], G[1][i], G[2][i], G[0][i], G[1][i], G[2][i]);
                const double beta = mp_dot3(G[0][j], G[1][j], G[2][j], G[0][j], G[1][j], G[2][j]);
                const double gamma = mp_dot3(G[0][i], G[1][i], G[2][i], G[0][j], G[1][j], G[2][j]);
                const double thr = np_dmul(np_dmul(2.0, kMlpnpEps), sqrt(np_dmul(alpha, beta)));
                if (!(fabs(gamma) > (thr > kMlpnpTiny ? thr : kMlpnpTiny))) continue;
                finished = false;
                double c, s, t;
                mp_jacobi(alpha, beta, gamma, c, s, t);
                for (int k = 0; k < 3; k++) {
                    const double gi = G[k][i], gj = G[k][j], vi = V[k][i], vj = V[k][j];
                    G[k][i] = np_dsub(np_dmul(c, gi), np_dmul(s, gj));
                    G[k][j] = np_dadd(np_dmul(s, gi), np_dmul(c, gj));
                    V[k][i] = np_dsub(np_dmul(c, vi), np_dmul(s, vj));
                    V[k][j] = np_dadd(np_dmul(s, vi), np_dmul(c, vj));
                }
            }
        if (finished) break;
    }
    for (int j = 0; j < 3; j++) {
        const double n = sqrt(mp_dot3(G[0][j], G[1][j], G[2][j], G[0][j], G[1][j], G[2][j]));
        for (int k = 0; k < 3; k++) G[k][j] = np_ddiv(G[k][j], n);
    }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rn[3 * r + c] = mp_dot3(G[r][0], G[r][1], G[r][2], V[c][0], V[c][1], V[c][2]);
}

// :703-718
NP_HD void mlpnp_rodrigues2rot(const double* w, double* R) {
    for (int i = 0; i < 9; i++) R[i] = (i % 4) == 0 ? 1.0 : 0.0;
    const double th = mp_norm3(w);
    if (th > kMlpnpEps) {
        const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
        const double a = np_ddiv(sin(th), th), b = np_ddiv(np_dsub(1.0, cos(th)), np_dmul(th, th));
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                const double kk = mp_dot3(K[3 * r], K[3 * r + 1], K[3 * r + 2], K[c], K[3 + c], K[6 + c]);
                R[3 * r + c] = np_dadd(np_dadd(R[3 * r + c], np_dmul(a, K[3 * r + c])), np_dmul(b, kk));
            }
    }
}

// :720-735
NP_HD void mlpnp_rot2rodrigues(const double* R, double* w) {
    w[0] = 0.0; w[1] = 0.0; w[2] = 0.0;
    const double trace = np_dsub(np_dadd(np_dadd(R[0], R[4]), R[8]), 1.0);
    const double wnorm = acos(np_ddiv(trace, 2.0));
    if (wnorm > kMlpnpEps) {
        const double sc = np_ddiv(wnorm, np_dmul(2.0, sin(wnorm)));
        w[0] = np_dmul(np_dsub(R[7], R[5]), sc);
        w[1] = np_dmul(np_dsub(R[2], R[6]), sc);
        w[2] = np_dmul(np_dsub(R[3], R[1]), sc);
    }
}

// r = n . u with u = q / |q|, q = R(w) p + T (:816-820), R = mlpnp_rodrigues2rot(w) handed in
NP_HD double mlpnp_residual(const double* R, const double* T, const double* p, const double* n) {
    double q[3];
    mp_mul3(R, p, q);
    for (int k = 0; k < 3; k++) q[k] = np_dadd(q[k], T[k]);
    const double nrm = mp_norm3(q);
    for (int k = 0; k < 3; k++) q[k] = np_ddiv(q[k], nrm);
    return mp_dot3(n[0], n[1], n[2], q[0], q[1], q[2]);
}

// The residual and its row of the Jacobian over (w, T).  For a change d of q:  d(n . u) = (n . d - (n . u)(u . d)) / |q|.
// dq/dT_k = e_k.  With th = |w|, a = sin th / th, b = (1 - cos th) / th^2, R p = p + a (w x p) + b (w x (w x p)):
//   dq/dw_k = (da/dth w_k / th) (w x p) + a (e_k x p) + (db/dth w_k / th) (w x (w x p)) + b (e_k x (w x p) + w x (e_k x p)),
//   da/dth = (th cos th - sin th) / th^2,   db/dth = (th sin th - 2 (1 - cos th)) / th^3.
// w_k / th is 0 / 0 at w = 0: the row is non-finite there.
NP_HD double mlpnp_residual_and_jacobian(const double* R, const double* w, const double* T, const double* p, const double* n, double* J) {
    double q[3], u[3];
    mp_mul3(R, p, q);
    for (int k = 0; k < 3; k++) q[k] = np_dadd(q[k], T[k]);
    const double nrm = mp_norm3(q);
    for (int k = 0; k < 3; k++) u[k] = np_ddiv(q[k], nrm);
    const double r = mp_dot3(n[0], n[1], n[2], u[0], u[1], u[2]);
    const double th = mp_norm3(w), sn = sin(th), cs = cos(th), th2 = np_dmul(th, th);
    const double a = np_ddiv(sn, th), b = np_ddiv(np_dsub(1.0, cs), th2);
    const double da = np_ddiv(np_dsub(np_dmul(th, cs), sn), th2);
    const double db = np_ddiv(np_dsub(np_dmul(th, sn), np_dmul(2.0, np_dsub(1.0, cs))), np_dmul(th2, th));
    double Kp[3], KKp[3];
    mp_cross(w, p, Kp);
    mp_cross(w, Kp, KKp);
    for (int k = 0; k < 3; k++) {
        const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        const double wk = np_ddiv(w[k], th), dak = np_dmul(da, wk), dbk = np_dmul(db, wk);
        double ep[3], eKp[3], wep[3], d[3];
        mp_cross(e, p, ep);
        mp_cross(e, Kp, eKp);
        mp_cross(w, ep, wep);
        for (int c = 0; c < 3; c++)
            d[c] = np_dadd(np_dadd(np_dadd(np_dmul(dak, Kp[c]), np_dmul(a, ep[c])), np_dmul(dbk, KKp[c])), np_dmul(b, np_dadd(eKp[c], wep[c])));
        const double nd = mp_dot3(n[0], n[1], n[2], d[0], d[1], d[2]), ud = mp_dot3(u[0], u[1], u[2], d[0], d[1], d[2]);
        J[k] = np_ddiv(np_dsub(nd, np_dmul(r, ud)), nrm);
        J[3 + k] = np_ddiv(np_dsub(n[k], np_dmul(r, u[k])), nrm);
    }
    return r;
}

// dx of S dx = g (S symmetric 6x6, row major): L D L^T without pivoting
NP_HD void mlpnp_solve6(const double (*S)[6], const double* g, double* dx) {
    double L[6][6], D[6], y[6];
    for (int j = 0; j < 6; j++) {
        double d = S[j][j];
        for (int k = 0; k < j; k++) d = np_dsub(d, np_dmul(np_dmul(L[j][k], L[j][k]), D[k]));
        D[j] = d;
        for (int i = j + 1; i < 6; i++) {
            double v = S[i][j];
            for (int k = 0; k < j; k++) v = np_dsub(v, np_dmul(np_dmul(L[i][k], L[j][k]), D[k]));
            L[i][j] = np_ddiv(v, d);
        }
    }
    for (int i = 0; i < 6; i++) {
        double v = g[i];
        for (int k = 0; k < i; k++) v = np_dsub(v, np_dmul(L[i][k], y[k]));
        y[i] = v;
    }
    for (int i = 5; i >= 0; i--) {
        double v = np_ddiv(y[i], D[i]);
        for (int k = i + 1; k < 6; k++) v = np_dsub(v, np_dmul(L[k][i], dx[k]));
        dx[i] = v;
    }
}

// sum over the six points of 1 - v . f, v = (R p + t) / |R p + t| (:625-629, :668-672)
NP_HD double mlpnp_direction_error(const MlpnpWork& w, const double* R, const double* t) {
    double sum = 0.0;
    for (int i = 0; i < 6; i++) {
        double v[3];
        mp_mul3(R, w.p[i], v);
        for (int k = 0; k < 3; k++) v[k] = np_dadd(v[k], t[k]);
        const double nrm = mp_norm3(v);
        for (int k = 0; k < 3; k++) v[k] = np_ddiv(v[k], nrm);
        sum = np_dadd(sum, np_dsub(1.0, mp_dot3(v[0], v[1], v[2], w.f[i][0], w.f[i][1], w.f[i][2])));
    }
    return sum;
}

// The right singular vector of the smallest singular value of the symmetric nc x nc matrix in w.W (nc = 12 or 9; W filled, V the
// identity, both synchronised by the caller): x[0..nc) = that column of V, x[nc..12) = 0.  Every lane returns the same x.
NP_HD void mlpnp_null_vector(MlpnpWork& w, int lane, int stride, int nc, double* x) {
    // :566-567 the cyclic Jacobi iteration: the rotation's c, s on every lane, row / column k of W and row k of V on lane k
    double max_diag = fabs(w.W[0][0]);
    for (int i = 1; i < nc; i++) if (fabs(w.W[i][i]) > max_diag) max_diag = fabs(w.W[i][i]);
    for (int sweep = 0; sweep < kMlpnpMaxSweeps; sweep++) {
        bool finished = true;
        for (int p = 0; p < nc - 1; p++)
            for (int q = p + 1; q < nc; q++) {
                const double apq = w.W[p][q], thr = np_dmul(np_dmul(2.0, kMlpnpEps), max_diag);
                if (!(fabs(apq) > (thr > kMlpnpTiny ? thr : kMlpnpTiny))) continue;   // the same on every lane
                finished = false;
                const double app = w.W[p][p], aqq = w.W[q][q];
                double c, s, tt;
                mp_jacobi(app, aqq, apq, c, s, tt);
                const double npp = np_dsub(app, np_dmul(tt, apq)), nqq = np_dadd(aqq, np_dmul(tt, apq));
                MLPNP_SYNC();
                for (int k = lane; k < nc; k += stride) {
                    if (k == p) { w.W[p][p] = npp; w.W[p][q] = 0.0; }
                    else if (k == q) { w.W[q][q] = nqq; w.W[q][p] = 0.0; }
                    else {
                        const double akp = w.W[k][p], akq = w.W[k][q];
                        const double nkp = np_dsub(np_dmul(c, akp), np_dmul(s, akq)), nkq = np_dadd(np_dmul(s, akp), np_dmul(c, akq));
                        w.W[k][p] = nkp; w.W[p][k] = nkp; w.W[k][q] = nkq; w.W[q][k] = nkq;
                    }
                    const double vkp = w.V[k][p], vkq = w.V[k][q];
                    w.V[k][p] = np_dsub(np_dmul(c, vkp), np_dmul(s, vkq));
                    w.V[k][q] = np_dadd(np_dmul(s, vkp), np_dmul(c, vkq));
                }
                MLPNP_SYNC();
                if (fabs(npp) > max_diag) max_diag = fabs(npp);
                if (fabs(nqq) > max_diag) max_diag = fabs(nqq);
            }
        if (finished) break;
    }
    int col = 0;
    for (int i = 1; i < nc; i++) if (fabs(w.W[i][i]) < fabs(w.W[col][col])) col = i;
    for (int k = 0; k < 12; k++) x[k] = k < nc ? w.V[k][col] : 0.0;
}

// computePose (:399-701) of the correspondences set[0..5] of a problem: cam = fx, fy, cx, cy; p2d (2 floats) and p3d (3 floats) per
// correspondence.  R (row major), t: the result block; returns the flags.  Every lane returns the same values.
NP_HD unsigned mlpnp_compute_pose(MlpnpWork& w, int lane, int stride, const float* cam, const float* p2d, const float* p3d, const int* set,
                                  double* R, double* t) {
    // :78-80 Pinhole::unproject in float, / z (= 1), widened; :410-418 the nullspaces
    for (int i = lane; i < 6; i += stride) {
        const int idx = set[i];
        const float bx = np_div(np_div(np_sub(p2d[2 * (size_t)idx], cam[2]), cam[0]), 1.0f);
        const float by = np_div(np_div(np_sub(p2d[2 * (size_t)idx + 1], cam[3]), cam[1]), 1.0f);
        w.f[i][0] = (double)bx; w.f[i][1] = (double)by; w.f[i][2] = 1.0;
        for (int k = 0; k < 3; k++) w.p[i][k] = (double)p3d[3 * (size_t)idx + k];
        const double nrm = mp_norm3(w.f[i]);
        const double nx = np_ddiv(w.f[i][0], nrm), ny = np_ddiv(w.f[i][1], nrm), nz = np_ddiv(w.f[i][2], nrm);
        const double s = nz >= 0.0 ? 1.0 : -1.0, a = np_ddiv(-1.0, np_dadd(s, nz)), b = np_dmul(np_dmul(nx, ny), a);
        w.ns[i][0][0] = np_dadd(1.0, np_dmul(np_dmul(s, np_dmul(nx, nx)), a));
        w.ns[i][0][1] = np_dmul(s, b);
        w.ns[i][0][2] = np_dmul(-s, nx);
        w.ns[i][1][0] = b;
        w.ns[i][1][1] = np_dadd(s, np_dmul(np_dmul(ny, ny), a));
        w.ns[i][1][2] = -ny;
    }
    MLPNP_SYNC();
    // :424-442 the planarity test on the uncentred P P^T
    double M[9], E[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = np_dmul(w.p[0][r], w.p[0][c]);
            for (int i = 1; i < 6; i++) s = np_dadd(s, np_dmul(w.p[i][r], w.p[i][c]));
            M[3 * r + c] = s;
        }
    const bool planar = mlpnp_rank3(M) == 2;
    if (planar) mlpnp_eig3(M, E);
    for (int i = lane; i < 6; i += stride) {
        if (planar) mp_mul3(E, w.p[i], w.q[i]);
        else for (int k = 0; k < 3; k++) w.q[i][k] = w.p[i][k];
    }
    MLPNP_SYNC();
    // :471-555 the design matrix, a row per lane
    const int nc = planar ? 9 : 12;
    for (int r = lane; r < 12; r += stride) {
        const int i = r >> 1;
        const double* n = w.ns[i][r & 1];
        for (int a = 0; a < 3; a++) {
            if (planar) {
                w.A[r][2 * a] = np_dmul(n[a], w.q[i][1]);
                w.A[r][2 * a + 1] = np_dmul(n[a], w.q[i][2]);
                w.A[r][6 + a] = n[a];
            } else {
                for (int b = 0; b < 3; b++) w.A[r][3 * a + b] = np_dmul(n[a], w.q[i][b]);
                w.A[r][9 + a] = n[a];
            }
        }
    }
    MLPNP_SYNC();
    // :564 A^T A: the sums of the upper triangle, one per lane, over the rows in ascending order
    for (int e = lane; e < nc * nc; e += stride) {
        const int a = e / nc, b = e % nc;
        if (a <= b) {
            double s = np_dmul(w.A[0][a], w.A[0][b]);
            for (int r = 1; r < 12; r++) s = np_dadd(s, np_dmul(w.A[r][a], w.A[r][b]));
            w.W[a][b] = s;
            w.W[b][a] = s;
        }
        w.V[a][b] = a == b ? 1.0 : 0.0;
    }
    MLPNP_SYNC();
    double x[12];
    mlpnp_null_vector(w, lane, stride, nc, x);
    // :573-680 the rotation nearest to the estimate and the disambiguation over the six points
    double Rout[9], tout[3];
    if (planar) {
        // tmp before transposeInPlace: column 0 = column 1 x column 2 (:580-585); T = tmp^T
        const double c1[3] = {x[0], x[2], x[4]}, c2[3] = {x[1], x[3], x[5]};
        double c0[3];
        mp_cross(c1, c2, c0);
        const double T[9] = {c0[0], c0[1], c0[2], c1[0], c1[1], c1[2], c2[0], c2[1], c2[2]};
        // :587 the columns 1 and 2 of the TRANSPOSED matrix, as the reference has it
        const double k1[3] = {T[1], T[4], T[7]}, k2[3] = {T[2], T[5], T[8]};
        const double scale = np_ddiv(1.0, sqrt(fabs(np_dmul(mp_norm3(k1), mp_norm3(k2)))));
        double R1[9], Rb[9];
        mlpnp_nearest_rotation(T, R1);
        if (mp_det3(R1) < 0.0) for (int i = 0; i < 9; i++) R1[i] = np_dmul(R1[i], -1.0);
        // :595 eigenRot^T * Rout1, :598-601 transposed, negated, the third column flipped on a negative determinant
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) Rb[3 * r + c] = mp_dot3(E[r], E[3 + r], E[6 + r], R1[c], R1[3 + c], R1[6 + c]);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R1[3 * r + c] = np_dmul(Rb[3 * c + r], -1.0);
        if (mp_det3(R1) < 0.0) for (int r = 0; r < 3; r++) R1[3 * r + 2] = np_dmul(R1[3 * r + 2], -1.0);
        const double tp[3] = {np_dmul(scale, x[6]), np_dmul(scale, x[7]), np_dmul(scale, x[8])}, tm[3] = {-tp[0], -tp[1], -tp[2]};
        double R2[9];
        for (int r = 0; r < 3; r++) { R2[3 * r] = -R1[3 * r]; R2[3 * r + 1] = -R1[3 * r + 1]; R2[3 * r + 2] = R1[3 * r + 2]; }
        double best = mlpnp_direction_error(w, R1, tp);   // std::min_element: the first minimum
        int idx = 0;
        const double e1 = mlpnp_direction_error(w, R1, tm), e2 = mlpnp_direction_error(w, R2, tp), e3 = mlpnp_direction_error(w, R2, tm);
        if (e1 < best) { best = e1; idx = 1; }
        if (e2 < best) { best = e2; idx = 2; }
        if (e3 < best) { best = e3; idx = 3; }
        for (int i = 0; i < 9; i++) Rout[i] = idx < 2 ? R1[i] : R2[i];
        for (int i = 0; i < 3; i++) tout[i] = (idx & 1) ? tm[i] : tp[i];
    } else {
        const double T[9] = {x[0], x[3], x[6], x[1], x[4], x[7], x[2], x[5], x[8]};
        const double k0[3] = {x[0], x[1], x[2]}, k1[3] = {x[3], x[4], x[5]}, k2[3] = {x[6], x[7], x[8]};
        const double scale = np_ddiv(1.0, pow(fabs(np_dmul(np_dmul(mp_norm3(k0), mp_norm3(k1)), mp_norm3(k2))), 1.0 / 3.0));
        double Rn[9], Ri[9], t0[3], t1[3];
        mlpnp_nearest_rotation(T, Rn);
        if (mp_det3(Rn) < 0.0) for (int i = 0; i < 9; i++) Rn[i] = np_dmul(Rn[i], -1.0);
        const double ts[3] = {np_dmul(scale, x[9]), np_dmul(scale, x[10]), np_dmul(scale, x[11])};
        double tf[3];
        mp_mul3(Rn, ts, tf);
        // :667 the inverses of [Rn | tf] and [Rn | -tf]
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) Ri[3 * r + c] = Rn[3 * c + r];
        mp_mul3(Ri, tf, t1);
        for (int k = 0; k < 3; k++) t0[k] = -t1[k];
        const double e0 = mlpnp_direction_error(w, Ri, t0), e1 = mlpnp_direction_error(w, Ri, t1);
        for (int i = 0; i < 9; i++) Rout[i] = Ri[i];
        for (int i = 0; i < 3; i++) tout[i] = e0 < e1 ? t0[i] : t1[i];
    }
    // :685-694 Gauss-Newton over (omega, t)
    double xs[6];
    mlpnp_rot2rodrigues(Rout, xs);
    for (int k = 0; k < 3; k++) xs[3 + k] = tout[k];
    unsigned steps = 0, broke = 0;
    for (int it = 0; it < 5; it++) {
        double Rw[9];
        mlpnp_rodrigues2rot(xs, Rw);
        for (int r = lane; r < 12; r += stride) w.r[r] = mlpnp_residual_and_jacobian(Rw, xs, xs + 3, w.p[r >> 1], w.ns[r >> 1][r & 1], w.J[r]);
        MLPNP_SYNC();
        // :777-780 J^T J (upper triangle) and J^T r, one sum per lane over the rows in ascending order
        for (int e = lane; e < 42; e += stride) {
            const int a = e / 7, b = e % 7;
            if (b == 6) {
                double s = np_dmul(w.J[0][a], w.r[0]);
                for (int r = 1; r < 12; r++) s = np_dadd(s, np_dmul(w.J[r][a], w.r[r]));
                w.g[a] = s;
            } else if (a <= b) {
                double s = np_dmul(w.J[0][a], w.J[0][b]);
                for (int r = 1; r < 12; r++) s = np_dadd(s, np_dmul(w.J[r][a], w.J[r][b]));
                w.S[a][b] = s;
                w.S[b][a] = s;
            }
        }
        MLPNP_SYNC();
        double dx[6];
        mlpnp_solve6(w.S, w.g, dx);
        // maxCoeff / minCoeff keep the first element unless a later one compares greater / smaller (a NaN never does)
        double mx = fabs(dx[0]), mn = fabs(dx[0]);
        for (int k = 1; k < 6; k++) { if (fabs(dx[k]) > mx) mx = fabs(dx[k]); if (fabs(dx[k]) < mn) mn = fabs(dx[k]); }
        if (mx > 5.0 || mn > 1.0) { broke = 1; break; }   // every lane alike: no lane is left waiting at a later MLPNP_SYNC
        double dl = 0.0;
        for (int r = 0; r < 12; r++) {
            double s = np_dmul(w.J[r][0], dx[0]);
            for (int k = 1; k < 6; k++) s = np_dadd(s, np_dmul(w.J[r][k], dx[k]));
            if (r == 0 || fabs(s) > dl) dl = fabs(s);
        }
        for (int k = 0; k < 6; k++) xs[k] = np_dsub(xs[k], dx[k]);
        steps++;
        MLPNP_SYNC();   // the next step writes J and r
        if (dl < 1e-5) break;
    }
    mlpnp_rodrigues2rot(xs, R);
    for (int k = 0; k < 3; k++) t[k] = xs[3 + k];
    return (planar ? kMlpnpPlanar : 0u) | (steps << 1) | (broke ? kMlpnpBroke : 0u);
}

// One i of CheckInliers (:310-333): the double mRi / mti times the float coordinates summed in double and narrowed to float,
// Pinhole::project (Pinhole.cpp:43-49) and the error in float.  No depth test.
NP_HD bool mlpnp_is_inlier(const double* R, const double* t, const float* cam, const float* X, const float* p2d, float max_err) {
    float c[3];
    for (int r = 0; r < 3; r++)
        c[r] = (float)np_dadd(np_dadd(np_dadd(np_dmul(R[3 * r], (double)X[0]), np_dmul(R[3 * r + 1], (double)X[1])), np_dmul(R[3 * r + 2], (double)X[2])), t[r]);
    const float u = np_add(np_div(np_mul(cam[0], c[0]), c[2]), cam[2]);
    const float v = np_add(np_div(np_mul(cam[1], c[1]), c[2]), cam[3]);
    const float dx = np_sub(p2d[0], u), dy = np_sub(p2d[1], v);
    return np_add(np_mul(dx, dx), np_mul(dy, dy)) < max_err;
}

}  // namespace msorb
