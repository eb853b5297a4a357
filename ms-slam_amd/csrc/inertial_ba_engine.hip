// Optimizer::FullInertialBA (src/Optimizer.cc:366-756) and Optimizer::MergeInertialBA (:3918-4420) for pinhole KeyFrames without a
// second camera, in double like g2o: one host-driven engine for both.  The arithmetic is full_inertial_ba_device.h and
// merge_inertial_ba_device.h (and through them the item functions of local_inertial_ba_device.h), the same text a host compiler
// reads (tests/full_inertial_ba_main.cc, tests/merge_inertial_ba_main.cc); this file is the executors that spread the passes over
// the chip, the staging and the C entries.  What the two routines do differently is a Routine, below.  DESIGN.md sections 25, 26.
//
// The host drives the loop (eg::levenberg with the stop flag as its `stopped`) and reads 32 bytes back per linearisation and per
// trial: the cost, computeScale's sum and the solver's status.  Everything else stays on the device between the upload and the
// read-back of the result.
//
//   linearise   edges (one thread per visual / inertial edge) -> gather (per point, per entry of Hpp, per entry of A^T omega)
//               -> one workgroup: b, then the cost over 256 slots
//   trial       the square cleared, prepare (Dinv per point; H + lambda I: only the entries that can be non-zero) -> Schur (one
//               thread per row of a block pair) -> ldlt::launch -> update (one thread per vertex) -> edges at the trial copy
//               -> one workgroup: the cost and computeScale's sum
//   at the end  classify (MergeInertialBA): one thread per visual edge reads the chi2 the last trial left
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
#include "inertial_ba_host.h"
#include "ldlt_blocked.h"
#include "merge_inertial_ba_device.h"

using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::iba_host::Carve;
using msorb::iba_host::finite_all;
using namespace msorb::fiba;
namespace miba = msorb::miba;
namespace liba = msorb::liba;
namespace ldlt = msorb::ldlt;

namespace {

constexpr int kThreads = 256;      // = liba::kSlots: the one-workgroup kernels give every slot a thread
constexpr int kMaxBlocks = 2048;

static_assert(sizeof(msorb_fiba_problem) == 64, "msorb_fiba_problem as the Python mirror lays it out");
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
__global__ __launch_bounds__(kThreads) void inertial_ba_edges_kernel(const Work F, int s) {
    GridExec ex;
    pass_edges<FULL>(ex, F, s);
}
__global__ __launch_bounds__(kThreads) void inertial_ba_gather_kernel(const Work F) {
    GridExec ex;
    pass_gather(ex, F);
}
__global__ __launch_bounds__(kThreads) void inertial_ba_prepare_kernel(const Work F, double lambda) {
    GridExec ex;
    pass_prepare(ex, F, lambda);
}
__global__ __launch_bounds__(kThreads) void inertial_ba_schur_kernel(const Work F) {
    GridExec ex;
    pass_schur(ex, F);
}
__global__ __launch_bounds__(kThreads) void inertial_ba_update_kernel(const Work F, int from, int to, double lambda) {
    GridExec ex;
    pass_update(ex, F, from, to, lambda);
}
// one workgroup: b and the cost at copy s
__global__ __launch_bounds__(kThreads) void inertial_ba_linearised_kernel(const Work F, int s) {
    BlockExec ex;
    pass_rhs(ex, F, s);
    ex.barrier();
    group_cost(ex, F, s);
}
// one workgroup: the cost at the trial copy and computeScale's sum
__global__ __launch_bounds__(kThreads) void inertial_ba_trial_kernel(const Work F, int s) {
    BlockExec ex;
    group_cost(ex, F, s);
    group_scale(ex, F);
}
// MergeInertialBA: the flags, from the chi2 the last trial left
__global__ __launch_bounds__(kThreads) void inertial_ba_classify_kernel(const Work F, uint8_t* outlier) {
    GridExec ex;
    miba::pass_classify(ex, F, outlier);
}

int blocks_for(long items) { return (int)std::min<long>((items + kThreads - 1) / kThreads, kMaxBlocks); }

// What FullInertialBA and MergeInertialBA do differently.  Everything else that differs follows from msorb_fiba_problem, which
// MergeInertialBA runs with init = 0, no priors and its own iterations.
struct Routine {
    int id;                    // which entry's stage times a call leaves
    const char* prefix;        // of every error text
    const char* stages_env;    // the variable that switches the stage timers on
    int max_kind;              // 2, or 3: free poses without inertial vertices; the unknowns are numbered through inert_of_free /
                               // free_of_inert, a KeyFrame's output is miba::keyframe_result's and the first shared unknown is n
    double lambda_init;        // setUserLambdaInit
    int iterations;            // what problem.iterations = 0 stands for
    bool classify;             // edge_outlier and n_outliers; a loop that completed no iteration is status 3: nothing to classify
};
constexpr Routine kFull{0, "full_inertial_ba: ", "MSORB_FULL_INERTIAL_BA_STAGES", 2, 1e-5, 0, false};              // :382
constexpr Routine kMerge{1, "merge_inertial_ba: ", "MSORB_MERGE_INERTIAL_BA_STAGES", 3, miba::kLambdaInit, miba::kIterations, true};

// per-stage device time of the calling thread's last call of either entry; one pool of events
enum Stage { kLinearise, kAssemble, kSchur, kSolve, kTrial, kStages };
struct StageTimer {
    std::vector<hipEvent_t> pool;
    std::vector<int> stage;
    size_t used = 0;
    float ms[2][kStages] = {};
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
    hipError_t collect(int id) {
        for (float& m : ms[id]) m = 0;
        for (size_t i = 0; i + 1 < used; i += 2) {
            float t = 0;
            if (hipError_t err = hipEventElapsedTime(&t, pool[i], pool[i + 1])) return err;
            ms[id][stage[i]] += t;
        }
        return hipSuccess;
    }
};
thread_local StageTimer g_stages;   // (its events live until the process ends)
bool stages_on(const Routine& R) {
    static const bool on[2] = {[] { const char* e = getenv(kFull.stages_env); return e && e[0] == '1'; }(),
                               [] { const char* e = getenv(kMerge.stages_env); return e && e[0] == '1'; }()};
    return on[R.id];
}
int stage_ms(const Routine& R, float ms[5]) {
    if (!ms) return MSORB_E_ARG;
    for (int i = 0; i < kStages; i++) ms[i] = g_stages.ms[R.id][i];
    return stages_on(R) ? MSORB_OK : MSORB_E_ARG;
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
#define ENGINE_TRY(expr) do { if (bad((expr), #expr)) return MSORB_E_HIP; } while (0)
#define ENGINE_LAUNCH(kernel, items, ...)                                                               \
    do {                                                                                                \
        if ((items) > 0) {                                                                              \
            hipLaunchKernelGGL(kernel, dim3(blocks_for(items)), dim3(kThreads), 0, s, __VA_ARGS__);     \
            ENGINE_TRY(hipGetLastError());                                                              \
        }                                                                                               \
    } while (0)
#define ENGINE_STAGE(st) do { if (timed) ENGINE_TRY(g_stages.mark(st, s)); } while (0)
    const Res& res() const { return *reinterpret_cast<const Res*>(h_res); }
    int read_res() {
        ENGINE_TRY(hipMemcpyAsync(h_res, d_res, sizeof(Res), hipMemcpyDeviceToHost, s));
        ENGINE_TRY(hipStreamSynchronize(s));
        return 0;
    }
    long edge_items() const { return std::max<long>(F.L.E, F.L.NI); }
    int linearise(int cur, double& chi) {
        const liba::Work& W = F.L;
        ENGINE_STAGE(kLinearise);
        ENGINE_LAUNCH(inertial_ba_edges_kernel<true>, edge_items(), F, cur);
        ENGINE_LAUNCH(inertial_ba_gather_kernel, std::max<long>(std::max<long>(W.P, 27L * W.Kf), (long)W.NI * kJc * 9), F);
        hipLaunchKernelGGL(inertial_ba_linearised_kernel, dim3(1), dim3(kThreads), 0, s, F, cur);
        ENGINE_TRY(hipGetLastError());
        ENGINE_STAGE(kLinearise);
        if (int rc = read_res()) return rc;
        chi = res().chi;
        return 0;
    }
    int trial(int cur, double lambda, double& chi, double& scale, int& solved) {
        const liba::Work& W = F.L;
        ENGINE_STAGE(kAssemble);
        ENGINE_TRY(hipMemsetAsync(W.S, 0, square_bytes, s));   // the entries nothing lists, which the last factorisation filled
        ENGINE_LAUNCH(inertial_ba_prepare_kernel, std::max<long>(std::max<long>(W.P, W.n), prepare_tasks(F)), F, lambda);
        ENGINE_STAGE(kAssemble);
        ENGINE_STAGE(kSchur);
        ENGINE_LAUNCH(inertial_ba_schur_kernel, 6L * (W.n_pairs + W.Kf), F);
        ENGINE_STAGE(kSchur);
        ENGINE_STAGE(kSolve);
        ENGINE_TRY(ldlt::launch(S, s));
        ENGINE_STAGE(kSolve);
        ENGINE_STAGE(kTrial);
        ENGINE_LAUNCH(inertial_ba_update_kernel, (long)(F.init ? W.K : W.Kf) + W.P + 1, F, cur, cur ^ 1, lambda);   // pass_update's items
        ENGINE_LAUNCH(inertial_ba_edges_kernel<false>, edge_items(), F, cur ^ 1);
        hipLaunchKernelGGL(inertial_ba_trial_kernel, dim3(1), dim3(kThreads), 0, s, F, cur ^ 1);
        ENGINE_TRY(hipGetLastError());
        ENGINE_STAGE(kTrial);
        if (int rc = read_res()) return rc;
        chi = res().chi;
        scale = res().scale;
        solved = res().solver_ok;
        return 0;
    }
};

// One call of either routine.  edge_outlier: R.classify alone.  Nothing is written through an output pointer before the call has
// succeeded: a call that returns an error leaves every output as it was.
int run(const Routine& R, int device, const msorb_fiba_problem* p, int n_kf, const msorb_iba_keyframe* kfs, int n_inertial,
        const msorb_iba_inertial_edge* iedges, int n_points, const float* pos_w, int n_edges, const int* edge_kf, const int* edge_point,
        const float* xy, const float* u_right, const float* inv_sigma2, const volatile int* stop_flag, msorb_iba_keyframe_out* kf_out,
        float* pos_out, double* pos_d, uint8_t* edge_outlier, uint8_t* point_included, msorb_iba_result* r, float* elapsed_ms) {
    auto refuse_with = [&](int code, const std::string& what) {
        set_last_error(R.prefix + what);
        return code;
    };
    // ---- the refusals
    if (!p || !r) return refuse_with(MSORB_E_INVALID, "a null required pointer");
    if (n_kf < 0 || n_inertial < 0 || n_points < 0 || n_edges < 0 || p->iterations < 0) return refuse_with(MSORB_E_INVALID, "a negative count");
    if ((n_kf > 0 && (!kfs || !kf_out)) || (n_inertial > 0 && !iedges) || (n_points > 0 && (!pos_w || !pos_out || !point_included)) ||
        (n_edges > 0 && (!edge_kf || !edge_point || !xy || !u_right || !inv_sigma2 || (R.classify && !edge_outlier))))
        return refuse_with(MSORB_E_INVALID, "a null required pointer");
    if (p->init != 0 && p->init != 1) return refuse_with(MSORB_E_INVALID, "an unknown init (0 or 1)");
    const int K = n_kf, NI = n_inertial, init = p->init;
    const bool kind3 = R.max_kind == 3;
    if (!std::isfinite(p->prior_g) || !std::isfinite(p->prior_a) || !finite_all(p->bg0, 6))
        return refuse_with(MSORB_E_INVALID, "a non-finite value in the problem");
    if (!msorb::iba_host::inputs_finite(R.prefix, K, kfs, NI, iedges, n_points, pos_w, n_edges, xy, u_right, inv_sigma2)) return MSORB_E_INVALID;
    static thread_local Problem q;
    plan_problem(init, K, kfs, NI, iedges, n_points, n_edges, edge_kf, edge_point, q, R.max_kind);
    if (q.code) return refuse_with(q.code == 1 ? MSORB_E_INVALID : MSORB_E_CAPACITY, q.why);
    auto untouched = [&](int status) {   // g2o's "0 vertices to optimize" (:683-685, :4312-4314), or the stop flag
        if (elapsed_ms) *elapsed_ms = 0;
        std::memset(r, 0, sizeof *r);
        r->status = status;
        msorb::iba_host::repeat_inputs(K, kfs, n_points, pos_w, n_edges, kf_out, pos_out, pos_d, R.classify ? edge_outlier : nullptr,
                                       point_included);
        return MSORB_OK;
    };
    const bool nothing = K == 0 || (!init && q.Kf == 0);
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
    const size_t o_fp = c.take((size_t)n_fp * 4);
    const size_t o_iof = c.take(kind3 ? (size_t)Kf * 4 : 0), o_foi = c.take((size_t)Ki * 4);   // max_kind = 2: Ki = 0, nothing taken
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
    const size_t n_flags = R.classify ? (size_t)E : 0, o_out = c.take(n_flags);
    const size_t dev_bytes = c.at;
    // pinned: the upload, then [res | state | points | flags] for the read-backs
    Carve hc;
    hc.at = in_bytes;
    const size_t h_res = hc.take(sizeof(Res)), h_st = hc.take((size_t)K * vsz), h_pt = hc.take((size_t)P * 24), h_out = hc.take(n_flags);
    static thread_local ThreadScratch scr(true, 2);   // one block for both routines
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
    for (int i = 0; i < NI; i++) reinterpret_cast<msorb_iba_inertial_edge*>(h + o_ie)[i] = staged_edge(iedges[i], init);
    put(o_free, plan.free_of_kf.data(), (size_t)K * 4);
    put(o_kof, plan.kf_of_free.data(), (size_t)Kf * 4);
    put(o_ein, q.e_in.data(), (size_t)K * 4);
    put(o_eout, q.e_out.data(), (size_t)K * 4);
    put(o_fp, q.fp_edge.data(), (size_t)n_fp * 4);
    put(o_iof, q.inert_of_free.data(), q.inert_of_free.size() * 4);
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
        for (int k = 0; k < K; k++) initial_vertices(V[k], kfs[k], *p);
        double* X = reinterpret_cast<double*>(h + o_pt0);
        for (int i = 0; i < P; i++)
            for (int a = 0; a < 3; a++) X[3 * (size_t)i + a] = (double)pos_w[3 * (size_t)q.point_of[i] + a];   // :559, :4230: the float position widened
    }
    Backend be{};
    Work& F = be.F;
    liba::Work& W = F.L;
    W.K = K; W.Kf = Kf; W.P = P; W.E = E; W.NI = NI; W.n = n; W.n_pairs = n_pairs;
    W.shared_bias = init;
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
    F.init = init; F.per = init ? 3 : 9; F.nb = kind3 ? n : 9 * Kf; F.n_fp = n_fp; F.fp_edge = ip(o_fp);
    if (kind3) { F.inert_of_free = ip(o_iof); F.free_of_inert = ip(o_foi); }   // else both null: every free KeyFrame has inertial vertices
    F.prior_g = (double)p->prior_g; F.prior_a = (double)p->prior_a;   // :538, :544: the floats widened
    F.bias_kf = 0;
    if (!kind3)
        for (int k = 0; k < K; k++)
            if (kfs[k].kind != 2) F.bias_kf = k;
    F.res = reinterpret_cast<Res*>(d + o_res);
    be.S.n = n; be.S.S = W.S; be.S.b = W.bs; be.S.x = W.x;
    ldlt::carve_workspace(be.S, dp(o_ws));
    be.S.ok = &F.res->solver_ok;
    be.s = s; be.h_res = h + h_res; be.d_res = d + o_res; be.square_bytes = (size_t)n * n * 8;
    be.timed = stages_on(R);
    g_stages.used = 0;

    hipError_t err = hipSuccess;
    auto fail = [&](const char* what) {
        set_last_error(std::string(R.prefix) + what + ": " + hipGetErrorString(err));
        scr.release();
        return MSORB_E_HIP;
    };
#define ENGINE_HOST_TRY(expr) do { err = (expr); if (err != hipSuccess) return fail(#expr); } while (0)
    ENGINE_HOST_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    // the second copy of the state starts equal to the first (a KeyFrame without a row is never written again)
    if (K) ENGINE_HOST_TRY(hipMemcpyAsync(d + o_st1, d + o_st0, (size_t)K * vsz, hipMemcpyDeviceToDevice, s));
    ENGINE_HOST_TRY(hipMemsetAsync(d + o_x, 0, (size_t)n * 8, s));   // a failed first solve leaves x as it was: zero
    if (NI) ENGINE_HOST_TRY(hipMemsetAsync(d + o_il, 0, (size_t)NI * sizeof(liba::IEdgeLin), s));
    if (elapsed_ms) ENGINE_HOST_TRY(hipEventRecord(scr.ev[0], s));
    msorb::eg::Outcome o;
    const int rc = msorb::eg::levenberg(
        be, p->iterations > 0 ? p->iterations : R.iterations, q.n_active > 0, o, [&](Backend&) { return R.lambda_init; },
        [&] { return stop_flag && *stop_flag; });   // SparseOptimizer::terminate
    if (rc) {
        err = be.err;
        return fail(be.what);
    }
    if (R.classify && o.iterations == 0) {
        // The flag rose between the check above and optimize()'s first terminate(): the reference would classify errors that were
        // never computed.  Handed back as status 3, nothing moved.
        ENGINE_HOST_TRY(hipStreamSynchronize(s));
        return untouched(3);
    }
    const int cur = be.current;
    if (n_flags) {
        hipLaunchKernelGGL(inertial_ba_classify_kernel, dim3(blocks_for(E)), dim3(kThreads), 0, s, F, d + o_out);
        ENGINE_HOST_TRY(hipGetLastError());
    }
    if (elapsed_ms) ENGINE_HOST_TRY(hipEventRecord(scr.ev[1], s));
    if (K) ENGINE_HOST_TRY(hipMemcpyAsync(h + h_st, d + (cur ? o_st1 : o_st0), (size_t)K * vsz, hipMemcpyDeviceToHost, s));
    if (P) ENGINE_HOST_TRY(hipMemcpyAsync(h + h_pt, d + (cur ? o_pt1 : o_pt0), (size_t)P * 24, hipMemcpyDeviceToHost, s));
    if (n_flags) ENGINE_HOST_TRY(hipMemcpyAsync(h + h_out, d + o_out, n_flags, hipMemcpyDeviceToHost, s));
    ENGINE_HOST_TRY(hipStreamSynchronize(s));
    float ms = 0;
    if (elapsed_ms) ENGINE_HOST_TRY(hipEventElapsedTime(&ms, scr.ev[0], scr.ev[1]));
    if (be.timed) ENGINE_HOST_TRY(g_stages.collect(R.id));
#undef ENGINE_HOST_TRY
    if (elapsed_ms) *elapsed_ms = ms;   // the call has succeeded: the outputs
    std::memset(r, 0, sizeof *r);
    const msorb::pinert::Vertices* V = reinterpret_cast<const msorb::pinert::Vertices*>(h + h_st);
    for (int k = 0; k < K; k++) {
        if (kind3) miba::keyframe_result(kfs[k], plan.free_of_kf[k], V[k], kf_out[k]);
        else keyframe_result(kfs[k], V[k], init, kf_out[k]);
    }
    for (size_t i = 0; i < 3 * (size_t)n_points; i++) {
        pos_out[i] = pos_w[i];
        if (pos_d) pos_d[i] = (double)pos_w[i];
    }
    const double* X = reinterpret_cast<const double*>(h + h_pt);
    for (int i = 0; i < P; i++)
        for (int a = 0; a < 3; a++) {
            const size_t dst = 3 * (size_t)q.point_of[i] + a;
            pos_out[dst] = (float)X[3 * (size_t)i + a];   // :746, :4413
            if (pos_d) pos_d[dst] = X[3 * (size_t)i + a];
        }
    for (int i = 0; i < n_points; i++) point_included[i] = q.included[i];
    if (R.classify && n_edges) std::memset(edge_outlier, 0, (size_t)n_edges);
    for (size_t e = 0; e < n_flags; e++) {
        edge_outlier[q.edge_of[e]] = h[h_out + e];
        r->n_outliers += h[h_out + e];
    }
    r->status = 0;
    r->iterations = o.iterations;
    r->trials = o.trials;
    r->rejected_trials = o.rejected;
    r->chi2_initial = o.chi2_initial;
    r->chi2_final = o.chi2_final;
    r->lambda_final = o.lambda;
    r->reserved = o.solver_failures;   // trials whose factorisation met a pivot that was not positive
    return MSORB_OK;
}

}  // namespace

extern "C" int msorb_full_inertial_ba_capacity(int init) { return capacity(init != 0); }
extern "C" int msorb_full_inertial_ba_stage_ms(float ms[5]) { return stage_ms(kFull, ms); }
extern "C" int msorb_full_inertial_ba(int device, const msorb_fiba_problem* p, int n_kf, const msorb_iba_keyframe* kfs, int n_inertial,
                                      const msorb_iba_inertial_edge* iedges, int n_points, const float* pos_w, int n_edges,
                                      const int* edge_kf, const int* edge_point, const float* xy, const float* u_right,
                                      const float* inv_sigma2, const volatile int* stop_flag, msorb_iba_keyframe_out* kf_out,
                                      float* pos_out, double* pos_d, uint8_t* point_included, msorb_iba_result* r, float* elapsed_ms) {
    return run(kFull, device, p, n_kf, kfs, n_inertial, iedges, n_points, pos_w, n_edges, edge_kf, edge_point, xy, u_right, inv_sigma2,
               stop_flag, kf_out, pos_out, pos_d, nullptr, point_included, r, elapsed_ms);
}

extern "C" int msorb_merge_inertial_ba_capacity(void) { return miba::capacity(); }
extern "C" int msorb_merge_inertial_ba_stage_ms(float ms[5]) { return stage_ms(kMerge, ms); }
extern "C" int msorb_merge_inertial_ba(int device, const msorb_iba_problem* p, int n_kf, const msorb_iba_keyframe* kfs, int n_inertial,
                                       const msorb_iba_inertial_edge* iedges, int n_points, const float* pos_w, int n_edges,
                                       const int* edge_kf, const int* edge_point, const float* xy, const float* u_right,
                                       const float* inv_sigma2, const volatile int* stop_flag, msorb_iba_keyframe_out* kf_out,
                                       float* pos_out, double* pos_d, uint8_t* edge_outlier, uint8_t* point_included, msorb_iba_result* r,
                                       float* elapsed_ms) {
    msorb_fiba_problem full{};   // init = 0, no priors; large is ignored
    if (p) full.iterations = p->iterations;
    return run(kMerge, device, p ? &full : nullptr, n_kf, kfs, n_inertial, iedges, n_points, pos_w, n_edges, edge_kf, edge_point, xy,
               u_right, inv_sigma2, stop_flag, kf_out, pos_out, pos_d, edge_outlier, point_included, r, elapsed_ms);
}
