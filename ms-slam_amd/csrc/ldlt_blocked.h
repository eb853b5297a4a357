// Dense symmetric solve S x = b by a blocked, multi-workgroup L D L^T: square-root-free, unpivoted, natural order, right-looking
// over the lower triangle, panel width kNB.  DESIGN.md section 16 has the whole story.
//
// Every entry of S goes through the arithmetic of the column-by-column factorisation (ba_solve_kernel of bundle_adjustment.hip,
// ldlt_solve of tests/local_ba_cases.py): column m takes  l_im v_km  off entry (i, k), l = v / d_m by ONE reciprocal, v the
// column before the scaling, for m ascending and each subtraction rounded on its own.  Blocking changes who does a subtraction and
// when, not its operands or its place in the entry's sequence, so the factor equals the unblocked one bit for bit.  For that the
// unscaled columns are kept beside L: v11 (the diagonal block's) and v21 (the panel's rows).
//
//   diag      one workgroup factors the nb x nb diagonal block in LDS; a pivot !(d > 0) clears *ok
//   panel     one thread per row below the block: the row's kNB entries through the block's columns, L and v written
//   update    one workgroup per kTile x kTile tile of the trailing lower triangle: entry -= l_im v_km for the panel's m ascending
//   forward   L y = b: every workgroup solves the panel's unit triangle in LDS (the same bits in each), workgroup 0 keeps y / d,
//             each thread takes the panel's columns off one row below
//   backward  L^T x = y / d from the last panel: the transposed triangle in LDS, each thread takes the panel's columns
//             (descending) off one row above
//
// *ok: the first diag launch sets it, a failed pivot clears it, and every later launch returns at once when it is clear: x is not
// written, nothing is read back in between.  No atomics, one stream: two runs return the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace msorb {
namespace ldlt {

constexpr int kNB = 48;        // panel width (a multiple of 6: a panel never splits a KeyFrame's block)
constexpr int kTile = 48;      // edge of a trailing-update tile
constexpr int kThreads = 256;  // diag, update, forward, backward
constexpr int kRowThreads = 64;

struct Work {
    int n;
    double* S;         // n x n, row-major, the lower triangle read and factored in place
    const double* b;   // n
    double* x;         // n, written only when every pivot was positive
    double *rd, *v11, *v21, *y, *w;   // 1 / d [n]; unscaled columns [kNB * kNB], [n * kNB]; the two substitutions' vectors [n]
    int* ok;
};

// doubles of rd + v11 + v21 + y + w
inline size_t workspace_doubles(int n) { return 3 * (size_t)n + (size_t)kNB * kNB + (size_t)n * kNB; }
inline void carve_workspace(Work& W, double* p) {
    const size_t n = (size_t)W.n;
    W.rd = p; W.y = p + n; W.w = p + 2 * n; W.v11 = p + 3 * n; W.v21 = W.v11 + (size_t)kNB * kNB;
}

static __global__ __launch_bounds__(kThreads) void ldlt_diag_kernel(const Work W, int j0) {
    __shared__ double A[kNB][kNB + 1], V[kNB][kNB + 1];
    const int n = W.n, t = threadIdx.x, nb = min(kNB, n - j0);
    if (j0 > 0 && !*W.ok) return;   // (uniform)
    for (int q = t; q < nb * nb; q += kThreads) {
        const int i = q / nb, k = q % nb;
        if (k <= i) A[i][k] = W.S[(size_t)(j0 + i) * n + j0 + k];
    }
    __syncthreads();
    for (int j = 0; j < nb; j++) {
        const double d = A[j][j];   // (uniform: written before the last barrier)
        if (!(d > 0)) {
            if (t == 0) *W.ok = 0;
            return;
        }
        const double r = 1.0 / d;
        if (t == 0) W.rd[j0 + j] = r;
        for (int i = j + 1 + t; i < nb; i += kThreads) {
            const double s = A[i][j];
            V[i][j] = s;
            A[i][j] = s * r;
        }
        __syncthreads();
        for (int i = j + 1 + (t >> 4); i < nb; i += kThreads / 16)
            for (int k = j + 1 + (t & 15); k <= i; k += 16) A[i][k] -= A[i][j] * V[k][j];
        __syncthreads();
    }
    for (int q = t; q < nb * nb; q += kThreads) {
        const int i = q / nb, k = q % nb;
        if (k < i) {
            W.S[(size_t)(j0 + i) * n + j0 + k] = A[i][k];
            W.v11[i * kNB + k] = V[i][k];
        }
    }
    if (j0 == 0 && t == 0) *W.ok = 1;
}

// rows j0 + kNB ..: a full block lies above them
static __global__ __launch_bounds__(kRowThreads) void ldlt_panel_kernel(const Work W, int j0) {
    __shared__ double V[kNB][kNB], r[kNB];
    if (!*W.ok) return;
    const int n = W.n, t = threadIdx.x;
    for (int q = t; q < kNB * kNB; q += kRowThreads) V[q / kNB][q % kNB] = (q % kNB) < (q / kNB) ? W.v11[q] : 0.0;
    if (t < kNB) r[t] = W.rd[j0 + t];
    __syncthreads();
    const int i = j0 + kNB + blockIdx.x * kRowThreads + t;
    if (i >= n) return;
    double* row = W.S + (size_t)i * n + j0;
    double* vrow = W.v21 + (size_t)i * kNB;
    double a[kNB];
#pragma unroll
    for (int k = 0; k < kNB; k++) a[k] = row[k];
#pragma unroll
    for (int m = 0; m < kNB; m++) {
        const double v = a[m], l = v * r[m];
        vrow[m] = v;
        row[m] = l;
#pragma unroll
        for (int k = m + 1; k < kNB; k++) a[k] -= l * V[k][m];
    }
}

// grid (nt, nt) over the trailing square from j0 + kNB; the tiles above the diagonal return at once
static __global__ __launch_bounds__(kThreads) void ldlt_update_kernel(const Work W, int j0) {
    __shared__ double Ls[kNB][kTile + 1], Vs[kNB][kTile + 1];   // [m][row of the tile]; + 1: the staging writes walk m
    if (blockIdx.x > blockIdx.y || !*W.ok) return;
    const int n = W.n, t = threadIdx.x, r0 = j0 + kNB + blockIdx.y * kTile, c0 = j0 + kNB + blockIdx.x * kTile;
    for (int q = t; q < kTile * kNB; q += kThreads) {
        const int rr = q / kNB, m = q % kNB;
        Ls[m][rr] = r0 + rr < n ? W.S[(size_t)(r0 + rr) * n + j0 + m] : 0.0;
        Vs[m][rr] = c0 + rr < n ? W.v21[(size_t)(c0 + rr) * kNB + m] : 0.0;
    }
    __syncthreads();
    constexpr int kPer = kTile / 16;
    const int ty = t >> 4, tx = t & 15;
    double acc[kPer][kPer];
    bool valid[kPer][kPer];
#pragma unroll
    for (int a = 0; a < kPer; a++)
#pragma unroll
        for (int b = 0; b < kPer; b++) {
            const int gi = r0 + ty + 16 * a, gc = c0 + tx + 16 * b;
            valid[a][b] = gi < n && gc <= gi;
            acc[a][b] = valid[a][b] ? W.S[(size_t)gi * n + gc] : 0.0;
        }
#pragma unroll 4   // (unrolled in full the compiler hoists every LDS read of the loop and spills)
    for (int m = 0; m < kNB; m++) {
        double l[kPer], v[kPer];
#pragma unroll
        for (int a = 0; a < kPer; a++) { l[a] = Ls[m][ty + 16 * a]; v[a] = Vs[m][tx + 16 * a]; }
#pragma unroll
        for (int a = 0; a < kPer; a++)
#pragma unroll
            for (int b = 0; b < kPer; b++) acc[a][b] -= l[a] * v[b];
    }
#pragma unroll
    for (int a = 0; a < kPer; a++)
#pragma unroll
        for (int b = 0; b < kPer; b++)
            if (valid[a][b]) W.S[(size_t)(r0 + ty + 16 * a) * n + c0 + tx + 16 * b] = acc[a][b];
}

// the panel's unit triangle into LDS: L[i][k] for k < i
__device__ inline void load_triangle(const Work& W, int j0, int nb, double (*L)[kNB + 1]) {
    for (int q = threadIdx.x; q < nb * nb; q += kThreads) {
        const int i = q / nb, k = q % nb;
        if (k < i) L[i][k] = W.S[(size_t)(j0 + i) * W.n + j0 + k];
    }
}

// y[i] loses L[i][m] y[m] for m ascending, as the column-by-column substitution does
static __global__ __launch_bounds__(kThreads) void ldlt_forward_kernel(const Work W, int j0) {
    __shared__ double L[kNB][kNB + 1], yp[kNB];
    if (!*W.ok) return;
    const int n = W.n, t = threadIdx.x, nb = min(kNB, n - j0);
    load_triangle(W, j0, nb, L);
    if (t < nb) yp[t] = W.y[j0 + t];
    __syncthreads();
    for (int m = 0; m < nb; m++) {
        if (t > m && t < nb) yp[t] -= L[t][m] * yp[m];
        __syncthreads();
    }
    if (blockIdx.x == 0 && t < nb) W.w[j0 + t] = yp[t] * W.rd[j0 + t];
    const int i = j0 + kNB + blockIdx.x * kThreads + t;
    if (i >= n) return;
    const double* row = W.S + (size_t)i * n + j0;
    double acc = W.y[i];
    for (int m = 0; m < kNB; m++) acc -= row[m] * yp[m];
    W.y[i] = acc;
}

// x[i] = y[i] / d[i] - sum_m L[m][i] x[m], the columns taken from the last
static __global__ __launch_bounds__(kThreads) void ldlt_backward_kernel(const Work W, int j0) {
    __shared__ double L[kNB][kNB + 1], xp[kNB];
    if (!*W.ok) return;
    const int n = W.n, t = threadIdx.x, nb = min(kNB, n - j0);
    load_triangle(W, j0, nb, L);
    if (t < nb) xp[t] = W.w[j0 + t];
    __syncthreads();
    for (int m = nb - 1; m >= 0; m--) {
        if (t < m) xp[t] -= L[m][t] * xp[m];
        __syncthreads();
    }
    if (blockIdx.x == 0 && t < nb) W.x[j0 + t] = xp[t];
    const int i = blockIdx.x * kThreads + t;
    if (i >= j0) return;
    double acc = W.w[i];
    for (int m = nb - 1; m >= 0; m--) acc -= W.S[(size_t)(j0 + m) * n + i] * xp[m];
    W.w[i] = acc;
}

// the whole solve on stream s; S is overwritten, *W.ok tells whether x was written
inline hipError_t launch(const Work& W, hipStream_t s) {
    const int n = W.n;
    if (n <= 0) return hipSuccess;
    hipError_t err;
    for (int j0 = 0; j0 < n; j0 += kNB) {
        hipLaunchKernelGGL(ldlt_diag_kernel, dim3(1), dim3(kThreads), 0, s, W, j0);
        const int rows = n - (j0 + kNB);
        if (rows > 0) {
            hipLaunchKernelGGL(ldlt_panel_kernel, dim3((rows + kRowThreads - 1) / kRowThreads), dim3(kRowThreads), 0, s, W, j0);
            const int nt = (rows + kTile - 1) / kTile;
            hipLaunchKernelGGL(ldlt_update_kernel, dim3(nt, nt), dim3(kThreads), 0, s, W, j0);
        }
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    if ((err = hipMemcpyAsync(W.y, W.b, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s)) != hipSuccess) return err;
    for (int j0 = 0; j0 < n; j0 += kNB) {
        const int rows = n - (j0 + kNB);
        hipLaunchKernelGGL(ldlt_forward_kernel, dim3(rows > 0 ? (rows + kThreads - 1) / kThreads : 1), dim3(kThreads), 0, s, W, j0);
    }
    if ((err = hipGetLastError()) != hipSuccess) return err;
    for (int j0 = ((n - 1) / kNB) * kNB; j0 >= 0; j0 -= kNB)
        hipLaunchKernelGGL(ldlt_backward_kernel, dim3(j0 > 0 ? (j0 + kThreads - 1) / kThreads : 1), dim3(kThreads), 0, s, W, j0);
    return hipGetLastError();
}

}  // namespace ldlt
}  // namespace msorb
