// Optimizer::OptimizeEssentialGraph4DoF (src/Optimizer.cc:5174-5458) after the gathering loops: g2o's Levenberg-Marquardt over the
// 4-DoF pose graph of VertexPose4DoF / Edge4DoF, in double: what a loop closure runs on an inertial map.  The arithmetic is
// essential_graph4_device.h's, the Levenberg loop essential_graph_device.h's, the index lists essential_graph_plan.h's, the dense
// solve ldlt_blocked.h's.  DESIGN.md section 18 has the whole story; the kernels have the shape of essential_graph.hip's
// (section 17) and share no arithmetic with them: rotation matrices, not quaternions; a 26-double estimate that carries DR and
// the update counter; a weighted quadratic form.
//
// The host drives the loop (eg::levenberg) and reads 32 bytes back per linearisation and per trial: the cost, computeScale or
// the largest diagonal entry (computeLambdaInit), and the solver's status.
//
//   table       once per call: ExpSO3(0, 0, +delta), ExpSO3(0, 0, -delta), ExpSO3(0, 0, 0)
//   linearise   32 lanes per active edge, two edges per wavefront: lane l computes error vector l of the 17 (the base error, 8 with
//               vertex 0 perturbed, 8 with vertex 1; a fixed end's are skipped); the Jacobian columns are differences of lane pairs,
//               taken through LDS; the 44 entries of A^T O A, B^T O B, A^T O B, A^T (-O e), B^T (-O e) are dealt over the lanes and
//               written edge-major as planes of Ea doubles; the edge's chi2 goes to a per-edge array
//   gather      one wavefront per free vertex adds H_ii and b_i over its incident list (lane l takes entries l, l + 64, ...; xor
//               butterfly), one per distinct free-free pair adds H_ij over the pair's list; kept compact
//   assemble    per trial: S is zeroed, the compact blocks are scattered into its lower triangle, lambda goes on the diagonal
//   trial       ldlt::launch on n = 4 Kf; one thread per free vertex applies UpdateW to the second copy of the state (DR and its
//               carried) and returns its share of computeScale; one thread per edge computes the error at the trial state
//   reduce      one workgroup adds the per-edge costs in a fixed order, and either the per-vertex scales or, after a
//               linearisation, the largest |H(j, j)|
//
// No floating-point atomics: every sum walks an index list in a fixed order, two runs return the same bits.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/msorb.h"
#include "ba_kernels_device.h"   // Carve, the stage timer, block_sum_256
#include "essential_graph4_device.h"
#include "essential_graph_plan.h"
#include "hip_host.h"
#include "ldlt_blocked.h"

using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::ba::block_sum_256;
using msorb::ba::Carve;
using msorb::se3::shfl_xor_f64;
using namespace msorb::eg4;
namespace ldlt = msorb::ldlt;

namespace {

constexpr int kCapacity = 1792;   // free vertices: S is 7168^2 doubles = 411 MB
constexpr int kThreads = 256, kLanesPerEdge = 32, kEdgesPerBlock = kThreads / kLanesPerEdge;
constexpr int kHd = 10;           // compact diagonal record: the upper triangle of H_ii, row major
constexpr int kMeas = 12;         // dRij[9], dtij[3]
constexpr size_t kStateBytes = kState * 8;

struct Eg4Res {
    double chi, scale, max_diagonal;
    int solver_ok, pad;
};

struct Eg4Dev {
    int N, Kf, Ea, n, n_pairs;
    const msorb_eg4_vertex* vtx;
    const int *free_of_vertex, *vertex_of_free, *ev0, *ev1, *inc_begin, *inc_entry, *pair_begin, *pair_i, *pair_j, *pair_entry;
    const double* meas;   // [Ea][kMeas]
    double* tab;          // [kTable][9]
    double* state[2];     // the two copies of the estimates, kState per vertex
    double *lin, *chi, *Hd, *Hp, *b, *S, *x, *part_vtx;
    Eg4Res* res;
};

__global__ void eg4_table_kernel(const Eg4Dev A) {
    const int k = threadIdx.x;
    if (k < kTable) exp_so3(0.0, 0.0, k == 0 ? 1e-9 : k == 1 ? -1e-9 : 0.0, A.tab + 9 * k);   // base_binary_edge.hpp:147
}

// computeActiveErrors + activeRobustChi2 + buildSystem's per-edge part (levenberg.cpp:75-87)
__global__ __launch_bounds__(kThreads) void eg4_linearise_kernel(const Eg4Dev A, int s) {
    __shared__ double err[kEdgesPerBlock][kErrors * 6], J[kEdgesPerBlock][48];
    const int g = threadIdx.x / kLanesPerEdge, lane = threadIdx.x % kLanesPerEdge;
    const int a = blockIdx.x * kEdgesPerBlock + g;
    const bool live = a < A.Ea;
    bool free0 = false, free1 = false;
    if (live) {
        const int i0 = A.ev0[a], i1 = A.ev1[a];
        free0 = A.free_of_vertex[i0] >= 0; free1 = A.free_of_vertex[i1] >= 0;
        const bool wanted = lane == 0 || (lane < 9 && free0) || (lane >= 9 && lane < kErrors && free1);
        if (wanted) {
            const msorb_eg4_vertex &V0 = A.vtx[i0], &V1 = A.vtx[i1];
            const double *c0[3] = {V0.Rwb, V0.Rcb, V0.tcb}, *c1[3] = {V1.Rwb, V1.Rcb, V1.tcb};
            double e[6];
            edge_error_variant(A.tab, A.meas + kMeas * (size_t)a, A.state[s] + kState * (size_t)i0, c0,
                               A.state[s] + kState * (size_t)i1, c1, lane, e);
            for (int d = 0; d < 6; d++) err[g][6 * lane + d] = e[d];
            if (lane == 0) A.chi[a] = edge_chi2(e);
        }
    }
    __syncthreads();
    if (live)
        for (int q = lane; q < 48; q += kLanesPerEdge) {   // J[side][d][col]
            const int side = q / 24, d = (q % 24) / 4, col = q % 4;
            if (side ? free1 : free0) J[g][q] = jacobian_entry(err[g], side, d, col);
        }
    __syncthreads();
    if (!live) return;
    const size_t Ea = (size_t)A.Ea;
    for (int q = lane; q < kPlanes; q += kLanesPerEdge) {
        const bool uses0 = q < kHbb || (q >= kHab && q < kBb), uses1 = (q >= kHbb && q < kBa) || q >= kBb;
        if ((uses0 && !free0) || (uses1 && !free1)) continue;   // no Jacobian, no block for a fixed end (:65-66)
        A.lin[(size_t)q * Ea + a] = quadratic_term(J[g], err[g], q);
    }
}

// One wavefront per task.  Tasks [0, Kf): H_ii (upper triangle) and b_i of free vertex i over its incident list.  Tasks after
// them: H_ij of pair (i, j), i < j, over the pair's list; an entry whose edge runs j -> i adds the transposed term.
__global__ __launch_bounds__(kThreads) void eg4_gather_kernel(const Eg4Dev A) {
    const size_t Ea = (size_t)A.Ea;
    const int task = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (task >= A.Kf + A.n_pairs) return;
    if (task < A.Kf) {
        double S[kHd + 4];
#pragma unroll
        for (int q = 0; q < kHd + 4; q++) S[q] = 0;
        for (int m = A.inc_begin[task] + lane; m < A.inc_begin[task + 1]; m += 64) {
            const int entry = A.inc_entry[m], a = entry >> 1, side = entry & 1;
            const double* Hx = A.lin + (size_t)(side ? kHbb : kHaa) * Ea + a;
            const double* bx = A.lin + (size_t)(side ? kBb : kBa) * Ea + a;
#pragma unroll
            for (int q = 0; q < kHd; q++) S[q] += Hx[(size_t)q * Ea];
#pragma unroll
            for (int q = 0; q < 4; q++) S[kHd + q] += bx[(size_t)q * Ea];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int q = 0; q < kHd + 4; q++) S[q] += shfl_xor_f64(S[q], off);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < kHd; q++) A.Hd[kHd * (size_t)task + q] = S[q];
#pragma unroll
            for (int q = 0; q < 4; q++) A.b[4 * (size_t)task + q] = S[kHd + q];
        }
        return;
    }
    const int p = task - A.Kf;
    double T[16];
#pragma unroll
    for (int q = 0; q < 16; q++) T[q] = 0;
    for (int m = A.pair_begin[p] + lane; m < A.pair_begin[p + 1]; m += 64) {
        const int entry = A.pair_entry[m], a = entry >> 1;
        const double* H = A.lin + (size_t)kHab * Ea + a;
        if (entry & 1) {
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) T[4 * r + c] += H[(size_t)(4 * c + r) * Ea];
        } else {
#pragma unroll
            for (int q = 0; q < 16; q++) T[q] += H[(size_t)q * Ea];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int q = 0; q < 16; q++) T[q] += shfl_xor_f64(T[q], off);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < 16; q++) A.Hp[16 * (size_t)p + q] = T[q];
}

// S (zeroed before) <- the lower triangle of H + lambda I: one thread per entry of a compact block (16 per task: Kf diagonal
// blocks, then the pairs; block (i, j), i < j, lands transposed at rows 4 j, columns 4 i)
__global__ __launch_bounds__(kThreads) void eg4_scatter_kernel(const Eg4Dev A, double lambda) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int task = (int)(t / 16), q = (int)(t % 16), r = q / 4, c = q % 4;
    if (task >= A.Kf + A.n_pairs) return;
    const size_t n = (size_t)A.n;
    if (task < A.Kf) {
        if (c > r) return;
        double h = A.Hd[kHd * (size_t)task + upper4(c, r)];
        if (r == c) h += lambda;                                               // setLambda (block_solver.hpp:573-578)
        A.S[(size_t)(4 * task + r) * n + 4 * task + c] = h;
        return;
    }
    const int p = task - A.Kf, i = A.pair_i[p], j = A.pair_j[p];
    A.S[(size_t)(4 * j + c) * n + 4 * i + r] = A.Hp[16 * (size_t)p + q];
}

// SparseOptimizer::update of the state copy `from` into the copy `to` (sparse_optimizer.cpp:422-441), one thread per free vertex;
// each returns its terms of computeScale (levenberg.cpp:188-195)
__global__ __launch_bounds__(kThreads) void eg4_update_kernel(const Eg4Dev A, int from, int to, double lambda) {
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= A.Kf) return;
    const int k = A.vertex_of_free[v];
    double x[4], sc = 0, dR[9];
    for (int r = 0; r < 4; r++) x[r] = A.x[4 * (size_t)v + r];
    exp_so3(0.0, 0.0, x[0], dR);                                               // G2oTypes.h:179-186, G2oTypes.cc:229
    const msorb_eg4_vertex& V = A.vtx[k];
    update_w(A.state[from] + kState * (size_t)k, dR, x + 1, V.Rwb, V.Rcb, V.tcb, A.state[to] + kState * (size_t)k);
    for (int r = 0; r < 4; r++) sc += x[r] * (lambda * x[r] + A.b[4 * (size_t)v + r]);
    A.part_vtx[v] = sc;
}

// computeActiveErrors + chi2 at a state copy (levenberg.cpp:123-124), one thread per active edge
__global__ __launch_bounds__(kThreads) void eg4_errors_kernel(const Eg4Dev A, int s) {
    const int a = blockIdx.x * kThreads + threadIdx.x;
    if (a >= A.Ea) return;
    const double *s0 = A.state[s] + kState * (size_t)A.ev0[a], *s1 = A.state[s] + kState * (size_t)A.ev1[a];
    double e[6];
    edge_error(s0 + kRcw, s0 + kTcw, s1 + kRcw, s1 + kTcw, A.meas + kMeas * (size_t)a, e);
    A.chi[a] = edge_chi2(e);
}

// one workgroup: res->chi = the sum of the edges' chi2 (thread t takes a = t, t + 256, ...; then the workgroup's fixed tree);
// with_scale: res->scale = the sum of the vertices' shares in the same way; without (after a linearisation): res->max_diagonal =
// the largest |H(j, j)| over the free vertices (a maximum does not depend on the order it is taken in)
__global__ __launch_bounds__(kThreads) void eg4_reduce_kernel(const Eg4Dev A, int with_scale) {
    __shared__ double lds[kThreads / 64], big[kThreads];
    double c = 0;
    for (int a = threadIdx.x; a < A.Ea; a += kThreads) c += A.chi[a];
    c = block_sum_256(c, lds);
    if (threadIdx.x == 0) A.res->chi = c;
    if (!with_scale) {
        double m = 0;
        for (int q = threadIdx.x; q < 4 * A.Kf; q += kThreads) m = fmax(fabs(A.Hd[kHd * (size_t)(q / 4) + upper4(q % 4, q % 4)]), m);
        big[threadIdx.x] = m;
        __syncthreads();
        for (int off = kThreads / 2; off >= 1; off >>= 1) {
            if ((int)threadIdx.x < off) big[threadIdx.x] = fmax(big[threadIdx.x], big[threadIdx.x + off]);
            __syncthreads();
        }
        if (threadIdx.x == 0) A.res->max_diagonal = big[0];
        return;
    }
    double v = 0;
    for (int i = threadIdx.x; i < A.Kf; i += kThreads) v += A.part_vtx[i];
    __syncthreads();
    v = block_sum_256(v, lds);
    if (threadIdx.x == 0) A.res->scale = v;
}

struct DeviceBackend {
    Eg4Dev A;
    ldlt::Work W;
    hipStream_t s;
    uint8_t *h_res, *d_res;
    bool timed;
    hipError_t err = hipSuccess;
    const char* what = "";
    int current = 0;
    double max_diagonal = 0;   // at the last linearisation

#define EG_TRY(expr) do { err = (expr); if (err != hipSuccess) { what = #expr; return MSORB_E_HIP; } } while (0)
#define EG_LAUNCH(kernel, blocks, ...)                                                   \
    do {                                                                                 \
        if ((blocks) > 0) {                                                              \
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), 0, s, __VA_ARGS__); \
            EG_TRY(hipGetLastError());                                                   \
        }                                                                                \
    } while (0)
#define EG_STAGE(st) do { if (timed) EG_TRY(msorb::ba::g_stages.mark(st, s)); } while (0)
    int read_res() {
        EG_TRY(hipMemcpyAsync(h_res, d_res, sizeof(Eg4Res), hipMemcpyDeviceToHost, s));
        EG_TRY(hipStreamSynchronize(s));
        return 0;
    }
    const Eg4Res& res() const { return *reinterpret_cast<const Eg4Res*>(h_res); }
    int linearise(int cur, double& chi) {
        EG_STAGE(msorb::ba::kLinearise);
        EG_LAUNCH(eg4_linearise_kernel, (A.Ea + kEdgesPerBlock - 1) / kEdgesPerBlock, A, cur);
        EG_LAUNCH(eg4_gather_kernel, (A.Kf + A.n_pairs + 3) / 4, A);
        EG_LAUNCH(eg4_reduce_kernel, 1, A, 0);
        EG_STAGE(msorb::ba::kLinearise);
        if (int rc = read_res()) return rc;
        chi = res().chi;
        max_diagonal = res().max_diagonal;
        return 0;
    }
    int trial(int cur, double lambda, double& chi, double& scale, int& solved) {
        EG_STAGE(msorb::ba::kSchur);   // (the assemble stage)
        EG_TRY(hipMemsetAsync(A.S, 0, (size_t)A.n * A.n * 8, s));
        EG_LAUNCH(eg4_scatter_kernel, (int)(((int64_t)(A.Kf + A.n_pairs) * 16 + kThreads - 1) / kThreads), A, lambda);
        EG_STAGE(msorb::ba::kSchur);
        EG_STAGE(msorb::ba::kSolve);
        EG_TRY(ldlt::launch(W, s));
        EG_STAGE(msorb::ba::kSolve);
        EG_STAGE(msorb::ba::kTrial);
        EG_LAUNCH(eg4_update_kernel, (A.Kf + kThreads - 1) / kThreads, A, cur, cur ^ 1, lambda);   // push + update (:103, :115)
        EG_LAUNCH(eg4_errors_kernel, (A.Ea + kThreads - 1) / kThreads, A, cur ^ 1);               // :123-124
        EG_LAUNCH(eg4_reduce_kernel, 1, A, 1);
        EG_STAGE(msorb::ba::kTrial);
        if (int rc = read_res()) return rc;
        chi = res().chi;
        scale = res().scale;
        solved = res().solver_ok;
        return 0;
    }
};

}  // namespace

extern "C" int msorb_essential_graph4_capacity(void) { return kCapacity; }

extern "C" int msorb_essential_graph4_stage_ms(float ms[4]) {
    if (!ms) return MSORB_E_ARG;
    for (int i = 0; i < msorb::ba::kStages; i++) ms[i] = msorb::ba::g_stages.ms[i];
    return msorb::ba::stages_on() ? MSORB_OK : MSORB_E_ARG;
}

extern "C" int msorb_essential_graph4(int device, int n_vertices, const msorb_eg4_vertex* vertices, int n_edges, const int* edge_v0,
                                      const int* edge_v1, const double* measurements, int iterations, double* poses_out,
                                      msorb_eg4_result* r, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (!r || n_vertices < 0 || n_edges < 0 || iterations < 0) return MSORB_E_ARG;
    if ((n_vertices > 0 && (!vertices || !poses_out)) || (n_edges > 0 && (!edge_v0 || !edge_v1 || !measurements))) return MSORB_E_ARG;
    const int N = n_vertices;
    static thread_local std::vector<int> fixed;
    static thread_local msorb::EssentialGraphPlan plan;
    fixed.resize((size_t)N);
    for (int k = 0; k < N; k++) fixed[k] = vertices[k].fixed != 0;
    switch (msorb::build_essential_graph_plan(N, fixed.data(), n_edges, edge_v0, edge_v1, plan)) {
        case msorb::kEgPlanIndexOutOfRange: set_last_error("essential_graph4: an edge names a vertex out of range"); return MSORB_E_ARG;
        case msorb::kEgPlanSelfEdge: set_last_error("essential_graph4: an edge joins a vertex to itself"); return MSORB_E_ARG;
        default: break;
    }
    const int Kf = plan.Kf, Ea = plan.Ea, n = 4 * Kf, n_pairs = (int)plan.pair_i.size();
    if (Kf > kCapacity) {
        set_last_error("essential_graph4: more free vertices than msorb_essential_graph4_capacity()");
        return MSORB_E_CAPACITY;
    }
    auto copy_inputs = [&] {
        for (int k = 0; k < N; k++) {
            std::memcpy(poses_out + 12 * (size_t)k, vertices[k].Rcw, 72);
            std::memcpy(poses_out + 12 * (size_t)k + 9, vertices[k].tcw, 24);
        }
    };
    if (Ea == 0 || iterations == 0) {   // nothing to optimise: zero iterations, the poses as they came, nothing launched
        std::memset(r, 0, sizeof *r);
        copy_inputs();
        return MSORB_OK;
    }
    if (int rc = msorb::require_device(device)) return rc;

    // ---- the device block: [uploaded | state and workspaces | result]
    Carve c;
    const size_t o_vtx = c.take((size_t)N * sizeof(msorb_eg4_vertex)), o_free = c.take((size_t)N * 4), o_vof = c.take((size_t)Kf * 4);
    const size_t o_e0 = c.take((size_t)Ea * 4), o_e1 = c.take((size_t)Ea * 4), o_ib = c.take(((size_t)Kf + 1) * 4);
    const size_t o_ie = c.take(plan.inc_entry.size() * 4), o_pb = c.take(((size_t)n_pairs + 1) * 4), o_pi = c.take((size_t)n_pairs * 4);
    const size_t o_pj = c.take((size_t)n_pairs * 4), o_pe = c.take(plan.pair_entry.size() * 4), o_meas = c.take((size_t)Ea * kMeas * 8);
    const size_t o_st0 = c.take((size_t)N * kStateBytes);
    const size_t in_bytes = c.at;
    const size_t o_st1 = c.take((size_t)N * kStateBytes), o_tab = c.take(kTable * 72), o_lin = c.take((size_t)kPlanes * Ea * 8);
    const size_t o_chi = c.take((size_t)Ea * 8), o_hd = c.take((size_t)Kf * kHd * 8), o_hp = c.take((size_t)n_pairs * 16 * 8);
    const size_t o_S = c.take((size_t)n * n * 8), o_b = c.take((size_t)n * 8), o_x = c.take((size_t)n * 8);
    const size_t o_ws = c.take(ldlt::workspace_doubles(n) * 8), o_pv = c.take((size_t)Kf * 8), o_res = c.take(sizeof(Eg4Res));
    const size_t dev_bytes = c.at;
    Carve hc;
    hc.at = in_bytes;
    const size_t h_res = hc.take(sizeof(Eg4Res)), h_st = hc.take((size_t)N * kStateBytes);
    static thread_local ThreadScratch scr(true, 2);
    if (dev_bytes > scr.d.n) {   // the block has to grow (by 1.5x): a system that does not fit is a matter of capacity
        if (hipSetDevice(device) != hipSuccess) return MSORB_E_HIP;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && dev_bytes + dev_bytes / 2 + 16 > free_b + (scr.device == device ? scr.d.n : 0)) {
            set_last_error("essential_graph4: the device has no room for the system");
            return MSORB_E_CAPACITY;
        }
    }
    if (int rc = scr.acquire(device, dev_bytes, hc.at)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    hipStream_t s = scr.s;
    auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) std::memcpy(h + off, src, bytes); };
    put(o_vtx, vertices, (size_t)N * sizeof(msorb_eg4_vertex));
    put(o_free, plan.free_of_vertex.data(), (size_t)N * 4);
    put(o_vof, plan.vertex_of_free.data(), (size_t)Kf * 4);
    put(o_ib, plan.inc_begin.data(), ((size_t)Kf + 1) * 4);
    put(o_ie, plan.inc_entry.data(), plan.inc_entry.size() * 4);
    put(o_pb, plan.pair_begin.data(), ((size_t)n_pairs + 1) * 4);
    put(o_pi, plan.pair_i.data(), (size_t)n_pairs * 4);
    put(o_pj, plan.pair_j.data(), (size_t)n_pairs * 4);
    put(o_pe, plan.pair_entry.data(), plan.pair_entry.size() * 4);
    {
        int *h0 = reinterpret_cast<int*>(h + o_e0), *h1 = reinterpret_cast<int*>(h + o_e1);
        double* hm = reinterpret_cast<double*>(h + o_meas);
        for (int a = 0; a < Ea; a++) {   // the active edges, compacted
            const int e = plan.active_edge[a];
            h0[a] = edge_v0[e];
            h1[a] = edge_v1[e];
            std::memcpy(hm + kMeas * (size_t)a, measurements + kMeas * (size_t)e, kMeas * 8);
        }
        double* hs = reinterpret_cast<double*>(h + o_st0);
        for (int k = 0; k < N; k++) state_init(vertices[k].Rcw, vertices[k].tcw, vertices[k].twb, hs + kState * (size_t)k);
    }
    DeviceBackend be{};
    Eg4Dev& A = be.A;
    A.N = N; A.Kf = Kf; A.Ea = Ea; A.n = n; A.n_pairs = n_pairs;
    A.vtx = reinterpret_cast<const msorb_eg4_vertex*>(d + o_vtx);
    auto ip = [&](size_t off) { return reinterpret_cast<const int*>(d + off); };
    auto dp = [&](size_t off) { return reinterpret_cast<double*>(d + off); };
    A.free_of_vertex = ip(o_free); A.vertex_of_free = ip(o_vof); A.ev0 = ip(o_e0); A.ev1 = ip(o_e1); A.inc_begin = ip(o_ib);
    A.inc_entry = ip(o_ie); A.pair_begin = ip(o_pb); A.pair_i = ip(o_pi); A.pair_j = ip(o_pj); A.pair_entry = ip(o_pe);
    A.meas = dp(o_meas);
    A.tab = dp(o_tab);
    A.state[0] = dp(o_st0); A.state[1] = dp(o_st1);
    A.lin = dp(o_lin); A.chi = dp(o_chi); A.Hd = dp(o_hd); A.Hp = dp(o_hp); A.b = dp(o_b); A.S = dp(o_S); A.x = dp(o_x); A.part_vtx = dp(o_pv);
    A.res = reinterpret_cast<Eg4Res*>(d + o_res);
    be.W.n = n; be.W.S = A.S; be.W.b = A.b; be.W.x = A.x;
    ldlt::carve_workspace(be.W, dp(o_ws));
    be.W.ok = &A.res->solver_ok;
    be.s = s;
    be.h_res = h + h_res;
    be.d_res = d + o_res;
    be.timed = msorb::ba::stages_on();
    msorb::ba::g_stages.used = 0;

    hipError_t err = hipSuccess;
    auto fail = [&](const char* what) {
        set_last_error(std::string("essential_graph4: ") + what + ": " + hipGetErrorString(err));
        scr.release();
        return MSORB_E_HIP;
    };
#define EG_HOST_TRY(expr) do { err = (expr); if (err != hipSuccess) return fail(#expr); } while (0)
    EG_HOST_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    // the second copy of the state starts equal to the first (a fixed vertex, or one outside the system, is never written again)
    EG_HOST_TRY(hipMemcpyAsync(d + o_st1, d + o_st0, (size_t)N * kStateBytes, hipMemcpyDeviceToDevice, s));
    EG_HOST_TRY(hipMemsetAsync(d + o_x, 0, (size_t)n * 8, s));   // a failed first solve leaves x as it was: zero
    if (elapsed_ms) EG_HOST_TRY(hipEventRecord(scr.ev[0], s));
    hipLaunchKernelGGL(eg4_table_kernel, dim3(1), dim3(64), 0, s, A);
    EG_HOST_TRY(hipGetLastError());

    msorb::eg::Outcome o;
    if (int rc = msorb::eg::levenberg(be, iterations, true, o, [](DeviceBackend& b) { return lambda_init(b.max_diagonal); })) {
        err = be.err;
        return rc == MSORB_E_HIP ? fail(be.what) : rc;
    }
    const int cur = be.current;
    if (elapsed_ms) EG_HOST_TRY(hipEventRecord(scr.ev[1], s));
    EG_HOST_TRY(hipMemcpyAsync(h + h_st, d + (cur ? o_st1 : o_st0), (size_t)N * kStateBytes, hipMemcpyDeviceToHost, s));
    EG_HOST_TRY(hipStreamSynchronize(s));
    if (elapsed_ms) EG_HOST_TRY(hipEventElapsedTime(elapsed_ms, scr.ev[0], scr.ev[1]));
    if (be.timed) EG_HOST_TRY(msorb::ba::g_stages.collect());
#undef EG_HOST_TRY
#undef EG_STAGE
#undef EG_LAUNCH
#undef EG_TRY
    const double* hs = reinterpret_cast<const double*>(h + h_st);
    copy_inputs();
    for (int i = 0; i < Kf; i++) {   // a vertex outside the system repeats its input
        const int k = plan.vertex_of_free[i];
        std::memcpy(poses_out + 12 * (size_t)k, hs + kState * (size_t)k + kRcw, 96);   // Rcw[9], tcw[3] lie together
    }
    r->status = 0;
    r->iterations = o.iterations;
    r->trials = o.trials;
    r->rejected_trials = o.rejected;
    r->solver_failures = o.solver_failures;
    r->stop = o.stop;
    r->chi2_initial = o.chi2_initial;
    r->chi2_final = o.chi2_final;
    r->lambda_final = o.lambda;
    r->lambda_initial = o.lambda_initial;
    return MSORB_OK;
}
