// Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1410-1675 and :1677-1985) after the gathering loops: g2o's Levenberg-Marquardt
// over a 7-DoF pose graph of VertexSim3Expmap / EdgeSim3, in double.  The arithmetic is essential_graph_device.h's, the index lists
// are essential_graph_plan.h's, the dense solve is ldlt_blocked.h's.  DESIGN.md section 17 has the whole story.
//
// The host drives the loop (eg::levenberg) and reads 32 bytes back per linearisation and per trial: the cost, computeScale and
// the solver's status.  Everything else stays on the device between the upload and the read-back of the estimates.
//
//   table       once per call: the 15 transforms Sim3(+-delta e_d) and Sim3(0), the same for every edge and every iteration
//   linearise   32 lanes per active edge, two edges per wavefront: lane l computes error vector l of the 29 (the base error, 14
//               with vertex 0 perturbed, 14 with vertex 1; a fixed end's are skipped); the Jacobian columns are differences of lane
//               pairs, taken through LDS; the 119 entries of A^T A, B^T B, A^T B, A^T (-e), B^T (-e) are dealt over the lanes and
//               written edge-major as planes of Ea doubles; the edge's chi2 goes to a per-edge array
//   gather      one wavefront per free vertex adds H_ii and b_i over its incident list (lane l takes entries l, l + 64, ...; xor
//               butterfly), one per distinct free-free pair adds H_ij over the pair's list; kept compact
//   assemble    per trial: S is zeroed, the compact blocks are scattered into its lower triangle, lambda goes on the diagonal
//               (the in-place factorisation destroys S, so a rejected trial rebuilds it)
//   trial       ldlt::launch on n = 7 Kf; one thread per free vertex applies oplus to the second copy of the state and returns its
//               share of computeScale; one thread per edge computes the error at the trial state
//   reduce      one workgroup adds the per-edge costs and the per-vertex scales in a fixed order
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
#include "essential_graph_device.h"
#include "essential_graph_plan.h"
#include "hip_host.h"
#include "ldlt_blocked.h"

using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::ba::block_sum_256;
using msorb::ba::Carve;
using msorb::se3::shfl_xor_f64;
using namespace msorb::eg;
namespace ldlt = msorb::ldlt;

namespace {

constexpr int kCapacity = 1024;   // free vertices: S is 7168^2 doubles = 411 MB
constexpr int kThreads = 256, kLanesPerEdge = 32, kEdgesPerBlock = kThreads / kLanesPerEdge;
constexpr int kHd = 28;           // compact diagonal record: the upper triangle of H_ii, row major

struct EgRes {
    double chi, scale, unused;
    int solver_ok, pad;
};

struct EgDev {
    int N, Kf, Ea, n, n_pairs;
    const msorb_eg_vertex* vtx;
    const int *free_of_vertex, *vertex_of_free, *ev0, *ev1, *inc_begin, *inc_entry, *pair_begin, *pair_i, *pair_j, *pair_entry;
    const double* meas;   // [Ea][8]
    Sim3* tab;            // [kTable]
    double* state[2];     // the two copies of the estimates, 8 per vertex
    double *lin, *chi, *Hd, *Hp, *b, *S, *x, *part_vtx;
    EgRes* res;
};

__device__ inline Sim3 load_sim3(const double* p) { return Sim3{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]}; }

__global__ void eg_table_kernel(const EgDev A) {
    const int k = threadIdx.x;
    if (k < kTable) A.tab[k] = table_entry(k);
}

// computeActiveErrors + activeRobustChi2 + buildSystem's per-edge part (levenberg.cpp:75-87)
__global__ __launch_bounds__(kThreads) void eg_linearise_kernel(const EgDev A, int s) {
    __shared__ double err[kEdgesPerBlock][kErrors * 7], J[kEdgesPerBlock][98];
    const int g = threadIdx.x / kLanesPerEdge, lane = threadIdx.x % kLanesPerEdge;
    const int a = blockIdx.x * kEdgesPerBlock + g;
    const bool live = a < A.Ea;
    int i0 = 0, i1 = 0;
    bool free0 = false, free1 = false;
    if (live) {
        i0 = A.ev0[a]; i1 = A.ev1[a];
        free0 = A.free_of_vertex[i0] >= 0; free1 = A.free_of_vertex[i1] >= 0;
        const bool wanted = lane == 0 || (lane < 15 && free0) || (lane >= 15 && lane < kErrors && free1);
        if (wanted) {
            const Sim3 C = load_sim3(A.meas + 8 * (size_t)a);
            const Sim3 v0 = load_sim3(A.state[s] + 8 * (size_t)i0), v1 = load_sim3(A.state[s] + 8 * (size_t)i1);
            double e[7];
            edge_error_variant(A.tab, C, v0, v1, A.vtx[i0].fix_scale != 0, A.vtx[i1].fix_scale != 0, lane, e);
            for (int d = 0; d < 7; d++) err[g][7 * lane + d] = e[d];
            if (lane == 0) A.chi[a] = edge_chi2(e);
        }
    }
    __syncthreads();
    if (live)
        for (int q = lane; q < 98; q += kLanesPerEdge) {   // J[side][d][col]
            const int side = q / 49, d = (q % 49) / 7, col = q % 7;
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
__global__ __launch_bounds__(kThreads) void eg_gather_kernel(const EgDev A) {
    const size_t Ea = (size_t)A.Ea;
    const int task = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (task >= A.Kf + A.n_pairs) return;
    if (task < A.Kf) {
        double S[35];
#pragma unroll
        for (int q = 0; q < 35; q++) S[q] = 0;
        for (int m = A.inc_begin[task] + lane; m < A.inc_begin[task + 1]; m += 64) {
            const int entry = A.inc_entry[m], a = entry >> 1, side = entry & 1;
            const double* Hx = A.lin + (size_t)(side ? kHbb : kHaa) * Ea + a;
            const double* bx = A.lin + (size_t)(side ? kBb : kBa) * Ea + a;
#pragma unroll
            for (int q = 0; q < 28; q++) S[q] += Hx[(size_t)q * Ea];
#pragma unroll
            for (int q = 0; q < 7; q++) S[28 + q] += bx[(size_t)q * Ea];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int q = 0; q < 35; q++) S[q] += shfl_xor_f64(S[q], off);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < kHd; q++) A.Hd[kHd * (size_t)task + q] = S[q];
#pragma unroll
            for (int q = 0; q < 7; q++) A.b[7 * (size_t)task + q] = S[kHd + q];
        }
        return;
    }
    const int p = task - A.Kf;
    double T[49];
#pragma unroll
    for (int q = 0; q < 49; q++) T[q] = 0;
    for (int m = A.pair_begin[p] + lane; m < A.pair_begin[p + 1]; m += 64) {
        const int entry = A.pair_entry[m], a = entry >> 1;
        const double* H = A.lin + (size_t)kHab * Ea + a;
        if (entry & 1) {
#pragma unroll
            for (int r = 0; r < 7; r++)
#pragma unroll
                for (int c = 0; c < 7; c++) T[7 * r + c] += H[(size_t)(7 * c + r) * Ea];
        } else {
#pragma unroll
            for (int q = 0; q < 49; q++) T[q] += H[(size_t)q * Ea];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int q = 0; q < 49; q++) T[q] += shfl_xor_f64(T[q], off);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < 49; q++) A.Hp[49 * (size_t)p + q] = T[q];
}

// S (zeroed before) <- the lower triangle of H + lambda I: one thread per entry of a compact block (49 per task: Kf diagonal
// blocks, then the pairs; block (i, j), i < j, lands transposed at rows 7 j, columns 7 i)
__global__ __launch_bounds__(kThreads) void eg_scatter_kernel(const EgDev A, double lambda) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int task = (int)(t / 49), q = (int)(t % 49), r = q / 7, c = q % 7;
    if (task >= A.Kf + A.n_pairs) return;
    const size_t n = (size_t)A.n;
    if (task < A.Kf) {
        if (c > r) return;
        double h = A.Hd[kHd * (size_t)task + upper7(c, r)];
        if (r == c) h += lambda;                                               // setLambda (block_solver.hpp:573-578)
        A.S[(size_t)(7 * task + r) * n + 7 * task + c] = h;
        return;
    }
    const int p = task - A.Kf, i = A.pair_i[p], j = A.pair_j[p];
    A.S[(size_t)(7 * j + c) * n + 7 * i + r] = A.Hp[49 * (size_t)p + q];
}

// SparseOptimizer::update of the state copy `from` into the copy `to` (sparse_optimizer.cpp:422-441), one thread per free vertex;
// each returns its terms of computeScale (levenberg.cpp:188-195), which reads x after oplusImpl has zeroed update[6]
__global__ __launch_bounds__(kThreads) void eg_update_kernel(const EgDev A, int from, int to, double lambda) {
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= A.Kf) return;
    const int k = A.vertex_of_free[v];
    double x[7], sc = 0;
    for (int r = 0; r < 7; r++) x[r] = A.x[7 * (size_t)v + r];
    const Sim3 Nw = msorb::sim3opt::sim3_oplus(load_sim3(A.state[from] + 8 * (size_t)k), x, A.vtx[k].fix_scale != 0);
    for (int r = 0; r < 7; r++) sc += x[r] * (lambda * x[r] + A.b[7 * (size_t)v + r]);
    double* o = A.state[to] + 8 * (size_t)k;
    o[0] = Nw.qx; o[1] = Nw.qy; o[2] = Nw.qz; o[3] = Nw.qw; o[4] = Nw.tx; o[5] = Nw.ty; o[6] = Nw.tz; o[7] = Nw.s;
    A.part_vtx[v] = sc;
}

// computeActiveErrors + chi2 at a state copy (levenberg.cpp:123-124), one thread per active edge
__global__ __launch_bounds__(kThreads) void eg_errors_kernel(const EgDev A, int s) {
    const int a = blockIdx.x * kThreads + threadIdx.x;
    if (a >= A.Ea) return;
    double e[7];
    edge_error(load_sim3(A.meas + 8 * (size_t)a), load_sim3(A.state[s] + 8 * (size_t)A.ev0[a]),
               load_sim3(A.state[s] + 8 * (size_t)A.ev1[a]), e);
    A.chi[a] = edge_chi2(e);
}

// one workgroup: res->chi = the sum of the edges' chi2 (thread t takes a = t, t + 256, ...; then the workgroup's fixed tree);
// with_scale: res->scale = the sum of the vertices' shares in the same way
__global__ __launch_bounds__(kThreads) void eg_reduce_kernel(const EgDev A, int with_scale) {
    __shared__ double lds[kThreads / 64];
    double c = 0;
    for (int a = threadIdx.x; a < A.Ea; a += kThreads) c += A.chi[a];
    c = block_sum_256(c, lds);
    if (threadIdx.x == 0) A.res->chi = c;
    if (!with_scale) return;
    double v = 0;
    for (int i = threadIdx.x; i < A.Kf; i += kThreads) v += A.part_vtx[i];
    __syncthreads();
    v = block_sum_256(v, lds);
    if (threadIdx.x == 0) A.res->scale = v;
}

struct DeviceBackend {
    EgDev A;
    ldlt::Work W;
    hipStream_t s;
    uint8_t *h_res, *d_res;
    bool timed;
    hipError_t err = hipSuccess;
    const char* what = "";
    int current = 0;

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
        EG_TRY(hipMemcpyAsync(h_res, d_res, sizeof(EgRes), hipMemcpyDeviceToHost, s));
        EG_TRY(hipStreamSynchronize(s));
        return 0;
    }
    const EgRes& res() const { return *reinterpret_cast<const EgRes*>(h_res); }
    int linearise(int cur, double& chi) {
        EG_STAGE(msorb::ba::kLinearise);
        EG_LAUNCH(eg_linearise_kernel, (A.Ea + kEdgesPerBlock - 1) / kEdgesPerBlock, A, cur);
        EG_LAUNCH(eg_gather_kernel, (A.Kf + A.n_pairs + 3) / 4, A);
        EG_LAUNCH(eg_reduce_kernel, 1, A, 0);
        EG_STAGE(msorb::ba::kLinearise);
        if (int rc = read_res()) return rc;
        chi = res().chi;
        return 0;
    }
    int trial(int cur, double lambda, double& chi, double& scale, int& solved) {
        EG_STAGE(msorb::ba::kSchur);   // (the assemble stage)
        EG_TRY(hipMemsetAsync(A.S, 0, (size_t)A.n * A.n * 8, s));
        EG_LAUNCH(eg_scatter_kernel, (int)(((int64_t)(A.Kf + A.n_pairs) * 49 + kThreads - 1) / kThreads), A, lambda);
        EG_STAGE(msorb::ba::kSchur);
        EG_STAGE(msorb::ba::kSolve);
        EG_TRY(ldlt::launch(W, s));
        EG_STAGE(msorb::ba::kSolve);
        EG_STAGE(msorb::ba::kTrial);
        EG_LAUNCH(eg_update_kernel, (A.Kf + kThreads - 1) / kThreads, A, cur, cur ^ 1, lambda);   // push + update (:103, :115)
        EG_LAUNCH(eg_errors_kernel, (A.Ea + kThreads - 1) / kThreads, A, cur ^ 1);               // :123-124
        EG_LAUNCH(eg_reduce_kernel, 1, A, 1);
        EG_STAGE(msorb::ba::kTrial);
        if (int rc = read_res()) return rc;
        chi = res().chi;
        scale = res().scale;
        solved = res().solver_ok;
        return 0;
    }
};

}  // namespace

extern "C" int msorb_essential_graph_capacity(void) { return kCapacity; }

extern "C" int msorb_essential_graph_stage_ms(float ms[4]) {
    if (!ms) return MSORB_E_ARG;
    for (int i = 0; i < msorb::ba::kStages; i++) ms[i] = msorb::ba::g_stages.ms[i];
    return msorb::ba::stages_on() ? MSORB_OK : MSORB_E_ARG;
}

extern "C" int msorb_essential_graph(int device, int n_vertices, const msorb_eg_vertex* vertices, int n_edges, const int* edge_v0,
                                     const int* edge_v1, const double* measurements, int iterations, double* estimates_out,
                                     msorb_eg_result* r, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (!r || n_vertices < 0 || n_edges < 0 || iterations < 0) return MSORB_E_ARG;
    if ((n_vertices > 0 && (!vertices || !estimates_out)) || (n_edges > 0 && (!edge_v0 || !edge_v1 || !measurements))) return MSORB_E_ARG;
    const int N = n_vertices;
    static thread_local std::vector<int> fixed;
    static thread_local msorb::EssentialGraphPlan plan;
    fixed.resize((size_t)N);
    for (int k = 0; k < N; k++) fixed[k] = vertices[k].fixed != 0;
    switch (msorb::build_essential_graph_plan(N, fixed.data(), n_edges, edge_v0, edge_v1, plan)) {
        case msorb::kEgPlanIndexOutOfRange: set_last_error("essential_graph: an edge names a vertex out of range"); return MSORB_E_ARG;
        case msorb::kEgPlanSelfEdge: set_last_error("essential_graph: an edge joins a vertex to itself"); return MSORB_E_ARG;
        default: break;
    }
    const int Kf = plan.Kf, Ea = plan.Ea, n = 7 * Kf, n_pairs = (int)plan.pair_i.size();
    if (Kf > kCapacity) {
        set_last_error("essential_graph: more free vertices than msorb_essential_graph_capacity()");
        return MSORB_E_CAPACITY;
    }
    auto copy_inputs = [&] {
        for (int k = 0; k < N; k++) {
            double* o = estimates_out + 8 * (size_t)k;
            for (int a = 0; a < 4; a++) o[a] = vertices[k].q[a];
            for (int a = 0; a < 3; a++) o[4 + a] = vertices[k].t[a];
            o[7] = vertices[k].s;
        }
    };
    if (Ea == 0 || iterations == 0) {   // nothing to optimise: zero iterations, the estimates as they came, nothing launched
        std::memset(r, 0, sizeof *r);
        copy_inputs();
        return MSORB_OK;
    }
    if (int rc = msorb::require_device(device)) return rc;

    // ---- the device block: [uploaded | state and workspaces | result]
    Carve c;
    const size_t o_vtx = c.take((size_t)N * sizeof(msorb_eg_vertex)), o_free = c.take((size_t)N * 4), o_vof = c.take((size_t)Kf * 4);
    const size_t o_e0 = c.take((size_t)Ea * 4), o_e1 = c.take((size_t)Ea * 4), o_ib = c.take(((size_t)Kf + 1) * 4);
    const size_t o_ie = c.take(plan.inc_entry.size() * 4), o_pb = c.take(((size_t)n_pairs + 1) * 4), o_pi = c.take((size_t)n_pairs * 4);
    const size_t o_pj = c.take((size_t)n_pairs * 4), o_pe = c.take(plan.pair_entry.size() * 4), o_meas = c.take((size_t)Ea * 64);
    const size_t o_st0 = c.take((size_t)N * 64);
    const size_t in_bytes = c.at;
    const size_t o_st1 = c.take((size_t)N * 64), o_tab = c.take(kTable * sizeof(Sim3)), o_lin = c.take((size_t)kPlanes * Ea * 8);
    const size_t o_chi = c.take((size_t)Ea * 8), o_hd = c.take((size_t)Kf * kHd * 8), o_hp = c.take((size_t)n_pairs * 49 * 8);
    const size_t o_S = c.take((size_t)n * n * 8), o_b = c.take((size_t)n * 8), o_x = c.take((size_t)n * 8);
    const size_t o_ws = c.take(ldlt::workspace_doubles(n) * 8), o_pv = c.take((size_t)Kf * 8), o_res = c.take(sizeof(EgRes));
    const size_t dev_bytes = c.at;
    Carve hc;
    hc.at = in_bytes;
    const size_t h_res = hc.take(sizeof(EgRes)), h_st = hc.take((size_t)N * 64);
    static thread_local ThreadScratch scr(true, 2);
    if (dev_bytes > scr.d.n) {   // the block has to grow (by 1.5x): a system that does not fit is a matter of capacity
        if (hipSetDevice(device) != hipSuccess) return MSORB_E_HIP;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && dev_bytes + dev_bytes / 2 + 16 > free_b + (scr.device == device ? scr.d.n : 0)) {
            set_last_error("essential_graph: the device has no room for the system");
            return MSORB_E_CAPACITY;
        }
    }
    if (int rc = scr.acquire(device, dev_bytes, hc.at)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    hipStream_t s = scr.s;
    auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) std::memcpy(h + off, src, bytes); };
    put(o_vtx, vertices, (size_t)N * sizeof(msorb_eg_vertex));
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
            std::memcpy(hm + 8 * (size_t)a, measurements + 8 * (size_t)e, 64);
        }
        double* hs = reinterpret_cast<double*>(h + o_st0);
        for (int k = 0; k < N; k++) {
            for (int a = 0; a < 4; a++) hs[8 * (size_t)k + a] = vertices[k].q[a];
            for (int a = 0; a < 3; a++) hs[8 * (size_t)k + 4 + a] = vertices[k].t[a];
            hs[8 * (size_t)k + 7] = vertices[k].s;
        }
    }
    DeviceBackend be{};
    EgDev& A = be.A;
    A.N = N; A.Kf = Kf; A.Ea = Ea; A.n = n; A.n_pairs = n_pairs;
    A.vtx = reinterpret_cast<const msorb_eg_vertex*>(d + o_vtx);
    auto ip = [&](size_t off) { return reinterpret_cast<const int*>(d + off); };
    auto dp = [&](size_t off) { return reinterpret_cast<double*>(d + off); };
    A.free_of_vertex = ip(o_free); A.vertex_of_free = ip(o_vof); A.ev0 = ip(o_e0); A.ev1 = ip(o_e1); A.inc_begin = ip(o_ib);
    A.inc_entry = ip(o_ie); A.pair_begin = ip(o_pb); A.pair_i = ip(o_pi); A.pair_j = ip(o_pj); A.pair_entry = ip(o_pe);
    A.meas = dp(o_meas);
    A.tab = reinterpret_cast<Sim3*>(d + o_tab);
    A.state[0] = dp(o_st0); A.state[1] = dp(o_st1);
    A.lin = dp(o_lin); A.chi = dp(o_chi); A.Hd = dp(o_hd); A.Hp = dp(o_hp); A.b = dp(o_b); A.S = dp(o_S); A.x = dp(o_x); A.part_vtx = dp(o_pv);
    A.res = reinterpret_cast<EgRes*>(d + o_res);
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
        set_last_error(std::string("essential_graph: ") + what + ": " + hipGetErrorString(err));
        scr.release();
        return MSORB_E_HIP;
    };
#define EG_HOST_TRY(expr) do { err = (expr); if (err != hipSuccess) return fail(#expr); } while (0)
    EG_HOST_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    // the second copy of the state starts equal to the first (a fixed vertex, or one outside the system, is never written again)
    EG_HOST_TRY(hipMemcpyAsync(d + o_st1, d + o_st0, (size_t)N * 64, hipMemcpyDeviceToDevice, s));
    EG_HOST_TRY(hipMemsetAsync(d + o_x, 0, (size_t)n * 8, s));   // a failed first solve leaves x as it was: zero
    if (elapsed_ms) EG_HOST_TRY(hipEventRecord(scr.ev[0], s));
    hipLaunchKernelGGL(eg_table_kernel, dim3(1), dim3(64), 0, s, A);
    EG_HOST_TRY(hipGetLastError());

    Outcome o;
    if (int rc = levenberg(be, iterations, true, o)) {
        err = be.err;
        return rc == MSORB_E_HIP ? fail(be.what) : rc;
    }
    const int cur = be.current;
    if (elapsed_ms) EG_HOST_TRY(hipEventRecord(scr.ev[1], s));
    EG_HOST_TRY(hipMemcpyAsync(h + h_st, d + (cur ? o_st1 : o_st0), (size_t)N * 64, hipMemcpyDeviceToHost, s));
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
        std::memcpy(estimates_out + 8 * (size_t)k, hs + 8 * (size_t)k, 64);
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
    return MSORB_OK;
}
