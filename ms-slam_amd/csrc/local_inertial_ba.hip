// Optimizer::LocalInertialBA (src/Optimizer.cc:2431-2973) for pinhole KeyFrames without a second camera: the whole optimize() and
// the classification in ONE launch, in double like g2o.  The arithmetic is local_inertial_ba_device.h, the same text a host
// compiler reads (tests/local_inertial_ba_main.cc); this file is the executor that spreads its passes over a workgroup, the
// staging, and the C entry.  DESIGN.md section 24.
//
// One workgroup of 512 threads owns the call: there is no stop flag to poll (the reference installs it after optimize(),
// :2868-2869), so the host reads nothing back until the end, and a workgroup's barrier is the only ordering the passes need.  The
// state, the edge-major linearisation, the 15 Kf square system (at most 375 x 375) and the index lists of local_ba_plan.h live
// in global memory (L2 at these sizes).  Thread t takes the items t, t + 512, ... of every pass; an item's sum walks its list
// in ascending order whoever computes it.  No atomics: two runs give the same bits, and so does the host program.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "inertial_ba_host.h"
#include "local_ba_plan.h"
#include "local_inertial_ba_device.h"

using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;
using msorb::iba_host::Carve;
using msorb::iba_host::repeat_inputs;
using namespace msorb::liba;

namespace {

constexpr int kThreads = 512;

static_assert(sizeof(msorb_iba_keyframe) == 408 && sizeof(msorb_iba_inertial_edge) == 1080 && sizeof(msorb_iba_keyframe_out) == 352 &&
                  sizeof(msorb_iba_result) == 56 && sizeof(msorb_iba_problem) == 16,
              "the records of include/msorb.h as the Python mirror lays them out");

struct BlockExec {
    __device__ inline int tid() const { return threadIdx.x; }
    __device__ inline int stride() const { return kThreads; }
    __device__ inline void barrier() { __syncthreads(); }
};

__global__ __launch_bounds__(kThreads) void local_inertial_ba_kernel(const Work W, int* cur_out) {
    BlockExec ex;
    const int cur = optimize(ex, W);
    if (threadIdx.x == 0) *cur_out = cur;
}

int refuse(const char* what) {
    set_last_error(std::string("local_inertial_ba: ") + what);
    return MSORB_E_INVALID;
}
int not_handled(const char* what) {
    set_last_error(std::string("local_inertial_ba: ") + what);
    return MSORB_E_CAPACITY;
}

}  // namespace

extern "C" int msorb_local_inertial_ba_capacity(void) { return kCapacity; }

extern "C" int msorb_local_inertial_ba(int device, const msorb_iba_problem* p, int n_kf, const msorb_iba_keyframe* kfs, int n_inertial,
                                       const msorb_iba_inertial_edge* iedges, int n_points, const float* pos_w, const uint8_t* point_close,
                                       int n_edges, const int* edge_kf, const int* edge_point, const float* xy, const float* u_right,
                                       const float* inv_sigma2, msorb_iba_keyframe_out* kf_out, float* pos_out, double* pos_d,
                                       uint8_t* edge_outlier, msorb_iba_result* r, float* elapsed_ms) {
    // ---- the refusals: nothing is written before the last of them has passed
    if (!p || !r) return refuse("a null required pointer");
    if (n_kf < 0 || n_inertial < 0 || n_points < 0 || n_edges < 0 || p->iterations < 0) return refuse("a negative count");
    if ((n_kf > 0 && (!kfs || !kf_out)) || (n_inertial > 0 && !iedges) || (n_points > 0 && (!pos_w || !point_close || !pos_out)) ||
        (n_edges > 0 && (!edge_kf || !edge_point || !xy || !u_right || !inv_sigma2 || !edge_outlier)))
        return refuse("a null required pointer");
    const int K = n_kf, P = n_points, E = n_edges, NI = n_inertial;
    static thread_local std::vector<int> fixed, e_in, e_out;
    static thread_local msorb::LocalBaPlan plan;
    fixed.resize((size_t)K);
    for (int k = 0; k < K; k++) {
        if (kfs[k].kind < 0 || kfs[k].kind > 2) return refuse("an unknown kind (0 free, 1 fixed with inertial vertices, 2 fixed pose)");
        fixed[k] = kfs[k].kind != 0;
    }
    e_in.assign((size_t)K, -1);
    e_out.assign((size_t)K, -1);
    bool chains = true;
    for (int i = 0; i < NI; i++) {
        const msorb_iba_inertial_edge& e = iedges[i];
        const int a = e.pre.kf_prev, b = e.pre.kf_cur;
        if (a < 0 || a >= K || b < 0 || b >= K) return refuse("an inertial edge names a KeyFrame out of range");
        if (a == b) return refuse("an inertial edge from a KeyFrame to itself");
        if (kfs[a].kind == 2 || kfs[b].kind == 2) return refuse("an inertial edge on a KeyFrame without inertial vertices (kind 2)");
        if (e_out[a] >= 0 || e_in[b] >= 0) chains = false;
        e_out[a] = i;
        e_in[b] = i;
    }
    if (!msorb::iba_host::inputs_finite("local_inertial_ba: ", K, kfs, NI, iedges, P, pos_w, E, xy, u_right, inv_sigma2)) return MSORB_E_INVALID;
    switch (msorb::build_local_ba_plan(K, fixed.data(), P, E, edge_kf, edge_point, plan)) {
        case msorb::kPlanIndexOutOfRange: return refuse("an edge names a KeyFrame or a point out of range");
        case msorb::kPlanNotPointMajor: return refuse("the edges are not point-major");
        default: break;
    }
    if (chains) {   // no cycle: every edge is reached from a KeyFrame that has no incoming one
        int reached = 0;
        for (int k = 0; k < K; k++)
            if (e_in[k] < 0)
                for (int m = e_out[k]; m >= 0; m = e_out[iedges[m].pre.kf_cur]) reached++;
        chains = reached == NI;
    }
    if (!chains) return not_handled("the inertial edges do not form chains (one incoming and one outgoing edge per KeyFrame)");
    const int Kf = plan.Kf, n = 15 * Kf;
    if (Kf > kCapacity) return not_handled("more free KeyFrames than msorb_local_inertial_ba_capacity()");
    if (elapsed_ms) *elapsed_ms = 0;
    std::memset(r, 0, sizeof *r);
    if (Kf == 0 && E == 0) {   // g2o's "0 vertices to optimize": nothing moved
        r->status = 2;
        repeat_inputs(K, kfs, P, pos_w, E, kf_out, pos_out, pos_d, edge_outlier, nullptr);
        return MSORB_OK;
    }
    if (int rc = msorb::require_device(device)) return rc;

    // ---- the device block: [uploaded | workspaces | results]
    const int n_pairs = (int)plan.pair_i.size();
    const size_t n_entries = plan.pair_a.size();
    Carve c;
    const size_t o_kf = c.take((size_t)K * sizeof(msorb_iba_keyframe)), o_ie = c.take((size_t)NI * sizeof(msorb_iba_inertial_edge));
    const size_t o_free = c.take((size_t)K * 4), o_kof = c.take((size_t)Kf * 4), o_ein = c.take((size_t)K * 4), o_eout = c.take((size_t)K * 4);
    const size_t o_ekf = c.take((size_t)E * 4), o_ept = c.take((size_t)E * 4), o_pb = c.take(((size_t)P + 1) * 4);
    const size_t o_kb = c.take(((size_t)Kf + 1) * 4), o_ke = c.take(plan.kf_edge.size() * 4);
    const size_t o_prb = c.take(((size_t)n_pairs + 1) * 4), o_pi = c.take((size_t)n_pairs * 4), o_pj = c.take((size_t)n_pairs * 4);
    const size_t o_pa = c.take(n_entries * 4), o_pbb = c.take(n_entries * 4);
    const size_t o_xy = c.take((size_t)E * 8), o_ur = c.take((size_t)E * 4), o_w = c.take((size_t)E * 4), o_close = c.take((size_t)P);
    const size_t o_st0 = c.take((size_t)K * sizeof(msorb::pinert::Vertices)), o_pt0 = c.take((size_t)P * 24);
    const size_t o_st1 = c.take((size_t)K * sizeof(msorb::pinert::Vertices)), o_pt1 = c.take((size_t)P * 24);
    const size_t in_bytes = c.at;
    const size_t o_lin = c.take((size_t)kPlanes * E * 8), o_hpp = c.take((size_t)Kf * 27 * 8), o_hll = c.take((size_t)P * 72);
    const size_t o_dinv = c.take((size_t)P * 72), o_A = c.take((size_t)n * n * 8), o_bA = c.take((size_t)n * 8);
    const size_t o_S = c.take((size_t)n * n * 8), o_bs = c.take((size_t)n * 8), o_x = c.take((size_t)n * 8);
    const size_t o_cv = c.take((size_t)n * 8), o_cl = c.take((size_t)n * 8), o_y = c.take((size_t)n * 8), o_rd = c.take((size_t)n * 8);
    const size_t o_chi = c.take((size_t)E * 8), o_rho = c.take((size_t)E * 8), o_slots = c.take((size_t)kSlots * 8);
    const size_t o_pv = c.take(((size_t)Kf + P) * 8), o_il = c.take((size_t)NI * sizeof(IEdgeLin)), o_res = c.take(sizeof(Res));
    const size_t o_out = c.take(sizeof(msorb_iba_result)), o_cur = c.take(4), o_flag = c.take((size_t)E);
    const size_t dev_bytes = c.at;
    // pinned: the upload (both copies of the state included), then [result | cur | flags | state 0 | points 0 | state 1 | points 1]
    Carve hc;
    hc.at = in_bytes;
    const size_t h_out = hc.take(sizeof(msorb_iba_result)), h_cur = hc.take(4), h_flag = hc.take((size_t)E);
    const size_t h_back = hc.take(in_bytes - o_st0);
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(device, dev_bytes, hc.at)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    hipStream_t s = scr.s;
    auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) std::memcpy(h + off, src, bytes); };
    put(o_kf, kfs, (size_t)K * sizeof(msorb_iba_keyframe));
    for (int i = 0; i < NI; i++) reinterpret_cast<msorb_iba_inertial_edge*>(h + o_ie)[i] = staged_edge(iedges[i]);
    put(o_free, plan.free_of_kf.data(), (size_t)K * 4);
    put(o_kof, plan.kf_of_free.data(), (size_t)Kf * 4);
    put(o_ein, e_in.data(), (size_t)K * 4);
    put(o_eout, e_out.data(), (size_t)K * 4);
    put(o_ekf, edge_kf, (size_t)E * 4);
    put(o_ept, edge_point, (size_t)E * 4);
    put(o_pb, plan.point_begin.data(), ((size_t)P + 1) * 4);
    put(o_kb, plan.kf_begin.data(), ((size_t)Kf + 1) * 4);
    put(o_ke, plan.kf_edge.data(), plan.kf_edge.size() * 4);
    put(o_prb, plan.pair_begin.data(), ((size_t)n_pairs + 1) * 4);
    put(o_pi, plan.pair_i.data(), (size_t)n_pairs * 4);
    put(o_pj, plan.pair_j.data(), (size_t)n_pairs * 4);
    put(o_pa, plan.pair_a.data(), n_entries * 4);
    put(o_pbb, plan.pair_b.data(), n_entries * 4);
    put(o_xy, xy, (size_t)E * 8);
    put(o_ur, u_right, (size_t)E * 4);
    put(o_w, inv_sigma2, (size_t)E * 4);
    put(o_close, point_close, (size_t)P);
    for (int copy = 0; copy < 2; copy++) {   // a fixed KeyFrame is never written again: both copies start equal
        msorb::pinert::Vertices* V = reinterpret_cast<msorb::pinert::Vertices*>(h + (copy ? o_st1 : o_st0));
        std::memset(static_cast<void*>(V), 0, (size_t)K * sizeof(msorb::pinert::Vertices));
        for (int k = 0; k < K; k++) vertices_from(V[k], kfs[k]);
        double* X = reinterpret_cast<double*>(h + (copy ? o_pt1 : o_pt0));
        for (size_t i = 0; i < 3 * (size_t)P; i++) X[i] = (double)pos_w[i];   // :2741: the float position widened
    }
    Work W{};
    W.K = K; W.Kf = Kf; W.P = P; W.E = E; W.NI = NI; W.n = n; W.n_pairs = n_pairs;
    W.large = p->large != 0;
    W.max_it = p->iterations > 0 ? p->iterations : (W.large ? 4 : 10);   // :2435-2440
    auto ip = [&](size_t off) { return reinterpret_cast<const int*>(d + off); };
    auto dp = [&](size_t off) { return reinterpret_cast<double*>(d + off); };
    W.kf = reinterpret_cast<const msorb_iba_keyframe*>(d + o_kf);
    W.ie = reinterpret_cast<const msorb_iba_inertial_edge*>(d + o_ie);
    W.free_of_kf = ip(o_free); W.kf_of_free = ip(o_kof); W.e_in = ip(o_ein); W.e_out = ip(o_eout); W.edge_kf = ip(o_ekf);
    W.edge_pt = ip(o_ept); W.point_begin = ip(o_pb); W.kf_begin = ip(o_kb); W.kf_edge = ip(o_ke); W.pair_begin = ip(o_prb);
    W.pair_i = ip(o_pi); W.pair_j = ip(o_pj); W.pair_a = ip(o_pa); W.pair_b = ip(o_pbb);
    W.xy = reinterpret_cast<const float*>(d + o_xy); W.ur = reinterpret_cast<const float*>(d + o_ur);
    W.w = reinterpret_cast<const float*>(d + o_w); W.close = d + o_close;
    W.st[0] = reinterpret_cast<msorb::pinert::Vertices*>(d + o_st0); W.st[1] = reinterpret_cast<msorb::pinert::Vertices*>(d + o_st1);
    W.pt[0] = dp(o_pt0); W.pt[1] = dp(o_pt1);
    W.lin = dp(o_lin); W.Hpp = dp(o_hpp); W.Hll = dp(o_hll); W.Dinv = dp(o_dinv); W.A = dp(o_A); W.bA = dp(o_bA); W.S = dp(o_S);
    W.bs = dp(o_bs); W.x = dp(o_x); W.col_v = dp(o_cv); W.col_l = dp(o_cl); W.y = dp(o_y); W.rd = dp(o_rd); W.chi2 = dp(o_chi);
    W.rho0 = dp(o_rho); W.slots = dp(o_slots); W.part_vtx = dp(o_pv);
    W.il = reinterpret_cast<IEdgeLin*>(d + o_il);
    W.res = reinterpret_cast<Res*>(d + o_res);
    W.out = reinterpret_cast<msorb_iba_result*>(d + o_out);
    W.outlier = d + o_flag;

    hipError_t err = hipSuccess;
    auto fail = [&](const char* what) {
        set_last_error(std::string("local_inertial_ba: ") + what + ": " + hipGetErrorString(err));
        scr.release();
        return MSORB_E_HIP;
    };
#define IBA_TRY(expr) do { err = (expr); if (err != hipSuccess) return fail(#expr); } while (0)
    IBA_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    if (n) IBA_TRY(hipMemsetAsync(d + o_x, 0, (size_t)n * 8, s));   // a failed first solve leaves x as it was: zero
    if (elapsed_ms) IBA_TRY(hipEventRecord(scr.ev[0], s));
    hipLaunchKernelGGL(local_inertial_ba_kernel, dim3(1), dim3(kThreads), 0, s, W, reinterpret_cast<int*>(d + o_cur));
    IBA_TRY(hipGetLastError());
    if (elapsed_ms) IBA_TRY(hipEventRecord(scr.ev[1], s));
    IBA_TRY(hipMemcpyAsync(h + h_out, d + o_out, o_flag + up16((size_t)E) - o_out, hipMemcpyDeviceToHost, s));   // result | cur | flags
    IBA_TRY(hipMemcpyAsync(h + h_back, d + o_st0, in_bytes - o_st0, hipMemcpyDeviceToHost, s));
    IBA_TRY(hipStreamSynchronize(s));
    if (elapsed_ms) IBA_TRY(hipEventElapsedTime(elapsed_ms, scr.ev[0], scr.ev[1]));
#undef IBA_TRY
    *r = *reinterpret_cast<const msorb_iba_result*>(h + h_out);
    if (r->status == 1) {   // :2911-2915: the reference returns before it erases or writes anything
        repeat_inputs(K, kfs, P, pos_w, E, kf_out, pos_out, pos_d, edge_outlier, nullptr);
        return MSORB_OK;
    }
    const int cur = *reinterpret_cast<const int*>(h + h_cur) & 1;
    const msorb::pinert::Vertices* V = reinterpret_cast<const msorb::pinert::Vertices*>(h + h_back + (cur ? o_st1 - o_st0 : 0));
    const double* X = reinterpret_cast<const double*>(h + h_back + (cur ? o_pt1 : o_pt0) - o_st0);
    repeat_inputs(K, kfs, 0, nullptr, 0, kf_out, nullptr, nullptr, nullptr, nullptr);
    for (int k = 0; k < K; k++)
        if (!fixed[k]) keyframe_out(V[k], kf_out[k]);
    for (size_t i = 0; i < 3 * (size_t)P; i++) {
        pos_out[i] = (float)X[i];   // :2968
        if (pos_d) pos_d[i] = X[i];
    }
    int n_outliers = 0;
    for (int e = 0; e < E; e++) { edge_outlier[e] = h[h_flag + e]; n_outliers += edge_outlier[e] != 0; }
    r->n_outliers = n_outliers;
    return MSORB_OK;
}
