// Optimizer::MergeInertialBA (src/Optimizer.cc:3918-4420) for pinhole KeyFrames without a second camera: the welding bundle
// adjustment of two inertial maps, in double like g2o.  The arithmetic is merge_inertial_ba_device.h over the passes of
// full_inertial_ba_device.h, the same text a host compiler reads (tests/merge_inertial_ba_main.cc); this file is the executors that
// spread the passes over the chip, the staging and the C entry.  DESIGN.md section 26.
//
// The host drives the loop (eg::levenberg from lambda 1e3 with the stop flag as its `stopped`) and reads 32 bytes back per
// linearisation and per trial, as full_inertial_ba.hip does:
//
//   linearise   edges -> gather -> one workgroup: b, then the cost over 256 slots
//   trial       the square cleared, prepare -> Schur -> ldlt::launch -> update -> edges at the trial copy -> one workgroup: the cost
//               and computeScale's sum
//   at the end  classify: one thread per visual edge reads the chi2 the last trial left
//
// A pass is a grid-stride loop over items and an item's sum walks its list in ascending order whoever computes it; no atomics, no
// graphs, one stream: two calls return the same bits, and so does the host program.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "ldlt_blocked.h"
#include "merge_inertial_ba_device.h"

using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;
using namespace msorb::miba;
namespace fiba = msorb::fiba;
namespace liba = msorb::liba;
namespace ldlt = msorb::ldlt;

namespace {

constexpr int kThreads = 256;      // = liba::kSlots: the one-workgroup kernels give every slot a thread
constexpr int kMaxBlocks = 2048;

static_assert(kThreads == liba::kSlots, "a slot per thread");

struct GridExec {
    __device__ inline long tid() const { return (long)blockIdx.x * kThreads + threadIdx.x; }
    __device__ inline long stride() const { return (long)gridDim.x * kThreads; }
};
struct BlockExec {
    __device__ inline int tid() const { return threadIdx.x; }
    __device__ inline int stride() const { return kThreads; }
    __device__ inline void barrier() { __syncthreads(); }
};

template <bool FULL>
__global__ __launch_bounds__(kThreads) void miba_edges_kernel(const Work F, int s) {
    GridExec ex;
    fiba::pass_edges<FULL>(ex, F, s);
}
__global__ __launch_bounds__(kThreads) void miba_gather_kernel(const Work F) {
    GridExec ex;
    fiba::pass_gather(ex, F);
}
__global__ __launch_bounds__(kThreads) void miba_prepare_kernel(const Work F, double lambda) {
    GridExec ex;
    fiba::pass_prepare(ex, F, lambda);
}
__global__ __launch_bounds__(kThreads) void miba_schur_kernel(const Work F) {
    GridExec ex;
    fiba::pass_schur(ex, F);
}
__global__ __launch_bounds__(kThreads) void miba_update_kernel(const Work F, int from, int to, double lambda) {
    GridExec ex;
    fiba::pass_update(ex, F, from, to, lambda);
}
__global__ __launch_bounds__(kThreads) void miba_classify_kernel(const Work F, uint8_t* outlier) {
    GridExec ex;
    pass_classify(ex, F, outlier);
}
// one workgroup: b and the cost at copy s
__global__ __launch_bounds__(kThreads) void miba_linearised_kernel(const Work F, int s) {
    BlockExec ex;
    fiba::pass_rhs(ex, F, s);
    ex.barrier();
    fiba::group_cost(ex, F, s);
}
// one workgroup: the cost at the trial copy and computeScale's sum
__global__ __launch_bounds__(kThreads) void miba_trial_kernel(const Work F, int s) {
    BlockExec ex;
    fiba::group_cost(ex, F, s);
    fiba::group_scale(ex, F);
}

int blocks_for(long items) { return (int)std::min<long>((items + kThreads - 1) / kThreads, kMaxBlocks); }

struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += up16(bytes); return o; }
};

int refuse_with(int code, const std::string& what) {
    set_last_error("merge_inertial_ba: " + what);
    return code;
}

bool finite_all(const double* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}
bool finite_all(const float* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// per-stage device time of the calling thread's last call
enum Stage { kLinearise, kAssemble, kSchur, kSolve, kTrial, kStages };
struct StageTimer {
    std::vector<hipEvent_t> pool;
    std::vector<int> stage;
    size_t used = 0;
    float ms[kStages] = {0, 0, 0, 0, 0};
    hipError_t mark(int st, hipStream_t s) {   // called before and after a stage
        if (used == pool.size()) {
            hipEvent_t e;
            if (hipError_t err = hipEventCreate(&e)) return err;
            pool.push_back(e);
            stage.push_back(0);
        }
        stage[used] = st;
        return hipEventRecord(pool[used++], s);
    }
    hipError_t collect() {
        for (float& m : ms) m = 0;
        for (size_t i = 0; i + 1 < used; i += 2) {
            float t = 0;
            if (hipError_t err = hipEventElapsedTime(&t, pool[i], pool[i + 1])) return err;
            ms[stage[i]] += t;
        }
        return hipSuccess;
    }
};
thread_local StageTimer g_stages;   // (its events live until the process ends)
bool stages_on() {
    static const bool on = [] { const char* e = getenv("MSORB_MERGE_INERTIAL_BA_STAGES"); return e && e[0] == '1'; }();
    return on;
}

// status 2 and 3: every output repeats its input and no flag is set
void repeat_inputs(int K, const msorb_iba_keyframe* kfs, int P, const float* pos_w, int E, msorb_iba_keyframe_out* kf_out, float* pos_out,
                   double* pos_d, uint8_t* edge_outlier, uint8_t* point_included) {
    for (int k = 0; k < K; k++) {
        msorb::pinert::Vertices V;
        liba::vertices_from(V, kfs[k]);
        liba::keyframe_out(V, kf_out[k]);
    }
    for (size_t i = 0; i < 3 * (size_t)P; i++) {
        pos_out[i] = pos_w[i];
        if (pos_d) pos_d[i] = (double)pos_w[i];
    }
    if (P) std::memset(point_included, 0, (size_t)P);
    if (E) std::memset(edge_outlier, 0, (size_t)E);
}

// what eg::levenberg drives
struct Backend {
    Work F;
    ldlt::Work S;
    hipStream_t s;
    uint8_t *h_res, *d_res;
    size_t square_bytes;
    bool timed;
    int current = 0;
    hipError_t err = hipSuccess;
    const char* what = "";

    bool bad(hipError_t e, const char* w) { err = e; what = w; return e != hipSuccess; }
#define MIBA_TRY(expr) do { if (bad((expr), #expr)) return MSORB_E_HIP; } while (0)
#define MIBA_LAUNCH(kernel, items, ...)                                                                 \
    do {                                                                                                \
        if ((items) > 0) {                                                                              \
            hipLaunchKernelGGL(kernel, dim3(blocks_for(items)), dim3(kThreads), 0, s, __VA_ARGS__);     \
            MIBA_TRY(hipGetLastError());                                                                \
        }                                                                                               \
    } while (0)
#define MIBA_STAGE(st) do { if (timed) MIBA_TRY(g_stages.mark(st, s)); } while (0)
    const Res& res() const { return *reinterpret_cast<const Res*>(h_res); }
    int read_res() {
        MIBA_TRY(hipMemcpyAsync(h_res, d_res, sizeof(Res), hipMemcpyDeviceToHost, s));
        MIBA_TRY(hipStreamSynchronize(s));
        return 0;
    }
    long edge_items() const { return std::max<long>(F.L.E, F.L.NI); }
    int linearise(int cur, double& chi) {
        const liba::Work& W = F.L;
        MIBA_STAGE(kLinearise);
        MIBA_LAUNCH(miba_edges_kernel<true>, edge_items(), F, cur);
        MIBA_LAUNCH(miba_gather_kernel, std::max<long>(std::max<long>(W.P, 27L * W.Kf), (long)W.NI * liba::kJc * 9), F);
        hipLaunchKernelGGL(miba_linearised_kernel, dim3(1), dim3(kThreads), 0, s, F, cur);
        MIBA_TRY(hipGetLastError());
        MIBA_STAGE(kLinearise);
        if (int rc = read_res()) return rc;
        chi = res().chi;
        return 0;
    }
    int trial(int cur, double lambda, double& chi, double& scale, int& solved) {
        const liba::Work& W = F.L;
        MIBA_STAGE(kAssemble);
        MIBA_TRY(hipMemsetAsync(W.S, 0, square_bytes, s));   // the entries nothing lists, which the last factorisation filled
        MIBA_LAUNCH(miba_prepare_kernel, std::max<long>(std::max<long>(W.P, W.n), fiba::prepare_tasks(F)), F, lambda);
        MIBA_STAGE(kAssemble);
        MIBA_STAGE(kSchur);
        MIBA_LAUNCH(miba_schur_kernel, 6L * (W.n_pairs + W.Kf), F);
        MIBA_STAGE(kSchur);
        MIBA_STAGE(kSolve);
        MIBA_TRY(ldlt::launch(S, s));
        MIBA_STAGE(kSolve);
        MIBA_STAGE(kTrial);
        MIBA_LAUNCH(miba_update_kernel, (long)W.Kf + W.P + 1, F, cur, cur ^ 1, lambda);
        MIBA_LAUNCH(miba_edges_kernel<false>, edge_items(), F, cur ^ 1);
        hipLaunchKernelGGL(miba_trial_kernel, dim3(1), dim3(kThreads), 0, s, F, cur ^ 1);
        MIBA_TRY(hipGetLastError());
        MIBA_STAGE(kTrial);
        if (int rc = read_res()) return rc;
        chi = res().chi;
        scale = res().scale;
        solved = res().solver_ok;
        return 0;
    }
};

}  // namespace

extern "C" int msorb_merge_inertial_ba_capacity(void) { return capacity(); }

extern "C" int msorb_merge_inertial_ba_stage_ms(float ms[5]) {
    if (!ms) return MSORB_E_ARG;
    for (int i = 0; i < kStages; i++) ms[i] = g_stages.ms[i];
    return stages_on() ? MSORB_OK : MSORB_E_ARG;
}

extern "C" int msorb_merge_inertial_ba(int device, const msorb_iba_problem* p, int n_kf, const msorb_iba_keyframe* kfs, int n_inertial,
                                       const msorb_iba_inertial_edge* iedges, int n_points, const float* pos_w, int n_edges,
                                       const int* edge_kf, const int* edge_point, const float* xy, const float* u_right,
                                       const float* inv_sigma2, const volatile int* stop_flag, msorb_iba_keyframe_out* kf_out,
                                       float* pos_out, double* pos_d, uint8_t* edge_outlier, uint8_t* point_included, msorb_iba_result* r,
                                       float* elapsed_ms) {
    // ---- the refusals: nothing is written before the last of them has passed
    if (!p || !r) return refuse_with(MSORB_E_INVALID, "a null required pointer");
    if (n_kf < 0 || n_inertial < 0 || n_points < 0 || n_edges < 0 || p->iterations < 0) return refuse_with(MSORB_E_INVALID, "a negative count");
    if ((n_kf > 0 && (!kfs || !kf_out)) || (n_inertial > 0 && !iedges) || (n_points > 0 && (!pos_w || !pos_out || !point_included)) ||
        (n_edges > 0 && (!edge_kf || !edge_point || !xy || !u_right || !inv_sigma2 || !edge_outlier)))
        return refuse_with(MSORB_E_INVALID, "a null required pointer");
    const int K = n_kf, NI = n_inertial;
    for (int k = 0; k < K; k++)
        if (!finite_all(kfs[k].Rwb, 48) || !finite_all(&kfs[k].fx, (size_t)5)) return refuse_with(MSORB_E_INVALID, "a non-finite value in a KeyFrame");
    for (int i = 0; i < NI; i++)
        if (!finite_all(iedges[i].pre.dR, (size_t)67) || !finite_all(iedges[i].pre.info, 81) || !finite_all(iedges[i].info_gyro, 18))
            return refuse_with(MSORB_E_INVALID, "a non-finite value in an inertial edge");
    if (!finite_all(pos_w, 3 * (size_t)n_points) || !finite_all(xy, 2 * (size_t)n_edges) || !finite_all(u_right, (size_t)n_edges) ||
        !finite_all(inv_sigma2, (size_t)n_edges))
        return refuse_with(MSORB_E_INVALID, "a non-finite value in a point or an observation");
    static thread_local Problem q;
    plan_problem(K, kfs, NI, iedges, n_points, n_edges, edge_kf, edge_point, q);
    if (q.code) return refuse_with(q.code == 1 ? MSORB_E_INVALID : MSORB_E_CAPACITY, q.why);
    const bool nothing = q.Kf == 0;
    auto untouched = [&](int status) {   // g2o's "0 vertices to optimize"; :4312-4314
        if (elapsed_ms) *elapsed_ms = 0;
        std::memset(r, 0, sizeof *r);
        r->status = status;
        repeat_inputs(K, kfs, n_points, pos_w, n_edges, kf_out, pos_out, pos_d, edge_outlier, point_included);
        return MSORB_OK;
    };
    if (nothing || (stop_flag && *stop_flag)) return untouched(nothing ? 2 : 3);
    if (int rc = msorb::require_device(device)) return rc;

    // ---- the device block: [uploaded | second copy, workspaces | results]
    const msorb::LocalBaPlan& plan = q.plan;
    const int Kf = q.Kf, Ki = (int)q.free_of_inert.size(), n = q.n, P = q.P, E = q.E, n_pairs = (int)plan.pair_i.size(),
              n_fp = (int)q.fp_edge.size();
    const size_t n_entries = plan.pair_a.size(), vsz = sizeof(msorb::pinert::Vertices);
    Carve c;
    const size_t o_kf = c.take((size_t)K * sizeof(msorb_iba_keyframe)), o_ie = c.take((size_t)NI * sizeof(msorb_iba_inertial_edge));
    const size_t o_free = c.take((size_t)K * 4), o_kof = c.take((size_t)Kf * 4), o_ein = c.take((size_t)K * 4), o_eout = c.take((size_t)K * 4);
    const size_t o_fp = c.take((size_t)n_fp * 4), o_iof = c.take((size_t)Kf * 4), o_foi = c.take((size_t)Ki * 4);
    const size_t o_ekf = c.take((size_t)E * 4), o_ept = c.take((size_t)E * 4), o_pb = c.take(((size_t)P + 1) * 4);
    const size_t o_kb = c.take(((size_t)Kf + 1) * 4), o_ke = c.take(plan.kf_edge.size() * 4);
    const size_t o_prb = c.take(((size_t)n_pairs + 1) * 4), o_pi = c.take((size_t)n_pairs * 4), o_pj = c.take((size_t)n_pairs * 4);
    const size_t o_pa = c.take(n_entries * 4), o_pbb = c.take(n_entries * 4);
    const size_t o_xy = c.take((size_t)E * 8), o_ur = c.take((size_t)E * 4), o_w = c.take((size_t)E * 4);
    const size_t o_st0 = c.take((size_t)K * vsz), o_pt0 = c.take((size_t)P * 24);
    const size_t in_bytes = c.at;
    const size_t o_st1 = c.take((size_t)K * vsz), o_pt1 = c.take((size_t)P * 24);
    const size_t o_lin = c.take((size_t)liba::kPlanes * E * 8), o_hpp = c.take((size_t)Kf * 27 * 8), o_hll = c.take((size_t)P * 72);
    const size_t o_dinv = c.take((size_t)P * 72), o_bA = c.take((size_t)n * 8);
    const size_t o_S = c.take((size_t)n * n * 8), o_bs = c.take((size_t)n * 8), o_x = c.take((size_t)n * 8);
    const size_t o_ws = c.take(ldlt::workspace_doubles(n) * 8);
    const size_t o_chi = c.take((size_t)E * 8), o_rho = c.take((size_t)E * 8), o_slots = c.take((size_t)liba::kSlots * 8);
    const size_t o_pv = c.take(((size_t)Kf + P + 1) * 8), o_il = c.take((size_t)NI * sizeof(liba::IEdgeLin)), o_res = c.take(sizeof(Res));
    const size_t o_out = c.take((size_t)E);
    const size_t dev_bytes = c.at;
    // pinned: the upload, then [res | state | points | flags] for the read-backs
    Carve hc;
    hc.at = in_bytes;
    const size_t h_res = hc.take(sizeof(Res)), h_st = hc.take((size_t)K * vsz), h_pt = hc.take((size_t)P * 24), h_out = hc.take((size_t)E);
    static thread_local ThreadScratch scr(true, 2);
    if (dev_bytes > scr.d.n) {   // the block has to grow (by 1.5x): a reduced system that does not fit is a matter of capacity
        if (hipSetDevice(device) != hipSuccess) return MSORB_E_HIP;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && dev_bytes + dev_bytes / 2 + 16 > free_b + (scr.device == device ? scr.d.n : 0))
            return refuse_with(MSORB_E_CAPACITY, "the device has no room for the reduced system");
    }
    if (int rc = scr.acquire(device, dev_bytes, hc.at)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    hipStream_t s = scr.s;
    auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) std::memcpy(h + off, src, bytes); };
    put(o_kf, kfs, (size_t)K * sizeof(msorb_iba_keyframe));
    for (int i = 0; i < NI; i++) reinterpret_cast<msorb_iba_inertial_edge*>(h + o_ie)[i] = liba::staged_edge(iedges[i]);
    put(o_free, plan.free_of_kf.data(), (size_t)K * 4);
    put(o_kof, plan.kf_of_free.data(), (size_t)Kf * 4);
    put(o_ein, q.e_in.data(), (size_t)K * 4);
    put(o_eout, q.e_out.data(), (size_t)K * 4);
    put(o_fp, q.fp_edge.data(), (size_t)n_fp * 4);
    put(o_iof, q.inert_of_free.data(), (size_t)Kf * 4);
    put(o_foi, q.free_of_inert.data(), (size_t)Ki * 4);
    put(o_ekf, q.ekf.data(), (size_t)E * 4);
    put(o_ept, q.ept.data(), (size_t)E * 4);
    put(o_pb, plan.point_begin.data(), ((size_t)P + 1) * 4);
    put(o_kb, plan.kf_begin.data(), ((size_t)Kf + 1) * 4);
    put(o_ke, plan.kf_edge.data(), plan.kf_edge.size() * 4);
    put(o_prb, plan.pair_begin.data(), ((size_t)n_pairs + 1) * 4);
    put(o_pi, plan.pair_i.data(), (size_t)n_pairs * 4);
    put(o_pj, plan.pair_j.data(), (size_t)n_pairs * 4);
    put(o_pa, plan.pair_a.data(), n_entries * 4);
    put(o_pbb, plan.pair_b.data(), n_entries * 4);
    {
        float* hxy = reinterpret_cast<float*>(h + o_xy);
        float* hur = reinterpret_cast<float*>(h + o_ur);
        float* hw = reinterpret_cast<float*>(h + o_w);
        for (int e = 0; e < E; e++) {
            const size_t src = (size_t)q.edge_of[e];
            hxy[2 * (size_t)e] = xy[2 * src];
            hxy[2 * (size_t)e + 1] = xy[2 * src + 1];
            hur[e] = u_right[src];
            hw[e] = inv_sigma2[src];
        }
        msorb::pinert::Vertices* V = reinterpret_cast<msorb::pinert::Vertices*>(h + o_st0);
        std::memset(static_cast<void*>(V), 0, (size_t)K * vsz);
        for (int k = 0; k < K; k++) liba::vertices_from(V[k], kfs[k]);
        double* X = reinterpret_cast<double*>(h + o_pt0);
        for (int i = 0; i < P; i++)
            for (int a = 0; a < 3; a++) X[3 * (size_t)i + a] = (double)pos_w[3 * (size_t)q.point_of[i] + a];   // :4230: the float position widened
    }
    Backend be{};
    Work& F = be.F;
    liba::Work& W = F.L;
    W.K = K; W.Kf = Kf; W.P = P; W.E = E; W.NI = NI; W.n = n; W.n_pairs = n_pairs;
    W.shared_bias = 0;
    auto ip = [&](size_t off) { return reinterpret_cast<const int*>(d + off); };
    auto dp = [&](size_t off) { return reinterpret_cast<double*>(d + off); };
    W.kf = reinterpret_cast<const msorb_iba_keyframe*>(d + o_kf);
    W.ie = reinterpret_cast<const msorb_iba_inertial_edge*>(d + o_ie);
    W.free_of_kf = ip(o_free); W.kf_of_free = ip(o_kof); W.e_in = ip(o_ein); W.e_out = ip(o_eout); W.edge_kf = ip(o_ekf);
    W.edge_pt = ip(o_ept); W.point_begin = ip(o_pb); W.kf_begin = ip(o_kb); W.kf_edge = ip(o_ke); W.pair_begin = ip(o_prb);
    W.pair_i = ip(o_pi); W.pair_j = ip(o_pj); W.pair_a = ip(o_pa); W.pair_b = ip(o_pbb);
    W.xy = reinterpret_cast<const float*>(d + o_xy); W.ur = reinterpret_cast<const float*>(d + o_ur);
    W.w = reinterpret_cast<const float*>(d + o_w);
    W.st[0] = reinterpret_cast<msorb::pinert::Vertices*>(d + o_st0); W.st[1] = reinterpret_cast<msorb::pinert::Vertices*>(d + o_st1);
    W.pt[0] = dp(o_pt0); W.pt[1] = dp(o_pt1);
    W.lin = dp(o_lin); W.Hpp = dp(o_hpp); W.Hll = dp(o_hll); W.Dinv = dp(o_dinv); W.bA = dp(o_bA); W.S = dp(o_S);
    W.bs = dp(o_bs); W.x = dp(o_x); W.chi2 = dp(o_chi); W.rho0 = dp(o_rho); W.slots = dp(o_slots); W.part_vtx = dp(o_pv);
    W.il = reinterpret_cast<liba::IEdgeLin*>(d + o_il);
    F.init = 0; F.per = 9; F.nb = n; F.n_fp = n_fp; F.fp_edge = ip(o_fp);
    F.inert_of_free = ip(o_iof); F.free_of_inert = ip(o_foi);
    F.res = reinterpret_cast<Res*>(d + o_res);
    be.S.n = n; be.S.S = W.S; be.S.b = W.bs; be.S.x = W.x;
    ldlt::carve_workspace(be.S, dp(o_ws));
    be.S.ok = &F.res->solver_ok;
    be.s = s; be.h_res = h + h_res; be.d_res = d + o_res; be.square_bytes = (size_t)n * n * 8;
    be.timed = stages_on();
    g_stages.used = 0;

    hipError_t err = hipSuccess;
    auto fail = [&](const char* what) {
        set_last_error(std::string("merge_inertial_ba: ") + what + ": " + hipGetErrorString(err));
        scr.release();
        return MSORB_E_HIP;
    };
#define MIBA_HOST_TRY(expr) do { err = (expr); if (err != hipSuccess) return fail(#expr); } while (0)
    MIBA_HOST_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    // the second copy of the state starts equal to the first (a KeyFrame without a row is never written again)
    if (K) MIBA_HOST_TRY(hipMemcpyAsync(d + o_st1, d + o_st0, (size_t)K * vsz, hipMemcpyDeviceToDevice, s));
    MIBA_HOST_TRY(hipMemsetAsync(d + o_x, 0, (size_t)n * 8, s));   // a failed first solve leaves x as it was: zero
    if (NI) MIBA_HOST_TRY(hipMemsetAsync(d + o_il, 0, (size_t)NI * sizeof(liba::IEdgeLin), s));
    hipEvent_t ev0 = scr.ev[0], ev1 = scr.ev[1];
    MIBA_HOST_TRY(hipEventRecord(ev0, s));
    msorb::eg::Outcome o;
    const int rc = msorb::eg::levenberg(
        be, p->iterations > 0 ? p->iterations : kIterations, q.n_active > 0, o, [](Backend&) { return kLambdaInit; },   // :4047, :4317
        [&] { return stop_flag && *stop_flag; });                                                                     // SparseOptimizer::terminate
    if (rc) {
        err = be.err;
        return fail(be.what);
    }
    if (o.iterations == 0) {
        // The flag rose between the check above and optimize()'s first terminate(): the reference would classify errors that were
        // never computed.  Handed back as status 3, nothing moved.
        MIBA_HOST_TRY(hipStreamSynchronize(s));
        return untouched(3);
    }
    const int cur = be.current;
    if (E) {
        hipLaunchKernelGGL(miba_classify_kernel, dim3(blocks_for(E)), dim3(kThreads), 0, s, F, d + o_out);
        MIBA_HOST_TRY(hipGetLastError());
    }
    MIBA_HOST_TRY(hipEventRecord(ev1, s));
    if (K) MIBA_HOST_TRY(hipMemcpyAsync(h + h_st, d + (cur ? o_st1 : o_st0), (size_t)K * vsz, hipMemcpyDeviceToHost, s));
    if (P) MIBA_HOST_TRY(hipMemcpyAsync(h + h_pt, d + (cur ? o_pt1 : o_pt0), (size_t)P * 24, hipMemcpyDeviceToHost, s));
    if (E) MIBA_HOST_TRY(hipMemcpyAsync(h + h_out, d + o_out, (size_t)E, hipMemcpyDeviceToHost, s));
    MIBA_HOST_TRY(hipStreamSynchronize(s));
    float ms = 0;
    MIBA_HOST_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    if (be.timed) MIBA_HOST_TRY(g_stages.collect());
#undef MIBA_HOST_TRY
    if (elapsed_ms) *elapsed_ms = ms;
    std::memset(r, 0, sizeof *r);
    const msorb::pinert::Vertices* V = reinterpret_cast<const msorb::pinert::Vertices*>(h + h_st);
    for (int k = 0; k < K; k++) keyframe_result(kfs[k], plan.free_of_kf[k], V[k], kf_out[k]);
    for (size_t i = 0; i < 3 * (size_t)n_points; i++) {
        pos_out[i] = pos_w[i];
        if (pos_d) pos_d[i] = (double)pos_w[i];
    }
    const double* X = reinterpret_cast<const double*>(h + h_pt);
    for (int i = 0; i < P; i++)
        for (int a = 0; a < 3; a++) {
            const size_t dst = 3 * (size_t)q.point_of[i] + a;
            pos_out[dst] = (float)X[3 * (size_t)i + a];   // :4413
            if (pos_d) pos_d[dst] = X[3 * (size_t)i + a];
        }
    for (int i = 0; i < n_points; i++) point_included[i] = q.included[i];
    if (n_edges) std::memset(edge_outlier, 0, (size_t)n_edges);
    int n_out = 0;
    for (int e = 0; e < E; e++) {
        edge_outlier[q.edge_of[e]] = h[h_out + e];
        n_out += h[h_out + e];
    }
    r->status = 0;
    r->iterations = o.iterations;
    r->trials = o.trials;
    r->rejected_trials = o.rejected;
    r->n_outliers = n_out;
    r->chi2_initial = o.chi2_initial;
    r->chi2_final = o.chi2_final;
    r->lambda_final = o.lambda;
    r->reserved = o.solver_failures;   // trials whose factorisation met a pivot that was not positive
    return MSORB_OK;
}
