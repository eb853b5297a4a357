// Sim3Solver's RANSAC (src/Sim3Solver.cc:228-373) with every hypothesis evaluated at once: msorb_sim3_ransac_batch.
//
// The random draws of the reference do not depend on the data (:254-265), so the caller hands in the minimal sets of ALL iterations
// and the loop splits into a map and a scan:
//
//   sim3_hypotheses_kernel  one workgroup of 256 threads per (hypothesis, problem).  Every thread runs ComputeSim3 (:390-491) on
//                           the three correspondences redundantly: the Horn step is a dependent chain of Jacobi rotations on uniform data,
//                           a latency no second wavefront can shorten, so running it once and broadcasting through LDS would make
//                           three wavefronts wait at a barrier for exactly as long as they now spend computing, and add the round
//                           trip.  Then CheckInliers (:494-518): thread t takes the correspondences t, t + 256, ...; a wavefront's
//                           64 decisions are one __ballot word of the hypothesis' mask, its count the popcounts of its words; the
//                           four wavefront counts meet in LDS and thread 0 adds them in ascending order.  No atomics.
//   sim3_select_kernel      one wavefront per problem: the sequential rule of :344-366 (sim3_select.h) over the counts in
//                           hypothesis order, then the winner's record and mask copied into the block the host reads back.
//
// One upload, two launches, one read-back on the calling thread's scratch.  The selection is a launch of its own and not a
// "last workgroup" epilogue of the first: that needs an agent-scope release / acquire per workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "sim3_device.h"
#include "sim3_select.h"

namespace msorb {
hipError_t small_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);   // orb_kernels.hip
}
using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kSelectChunk = 1024;   // counts the selection stages in LDS at a time

static_assert(sizeof(msorb_sim3_problem) == 52 && sizeof(msorb_sim3_result) == 132, "the records of include/msorb.h as the Python mirror lays them out");

struct Sim3ProblemDev {
    msorb_sim3_problem p;
    int corr0, hyp0;                    // the problem's first correspondence / hypothesis in the flat arrays
    unsigned long long mask0, wmask0;   // its first mask word among all hypotheses' masks / among the winners' masks
};
struct Sim3Record { float s, R[9], t[3]; };

struct Sim3Args {
    const Sim3ProblemDev* prob;
    const int* hyp_problem;   // per hypothesis: its problem
    const int* triples;       // per hypothesis: three correspondence indices of its problem
    const float *X1, *X2, *max_err1, *max_err2;
    Sim3Record* rec;          // per hypothesis
    unsigned long long* mask; // per hypothesis ceil(n / 64) words
    int* counts;              // per hypothesis
    msorb_sim3_result* result;
    unsigned long long* wmask;   // per problem ceil(n / 64) words: the winner's mask
};

__global__ __launch_bounds__(kThreads) void sim3_hypotheses_kernel(const Sim3Args A) {
    __shared__ int wave_count[kWaves];
    const int g = blockIdx.x;
    const Sim3ProblemDev P = A.prob[A.hyp_problem[g]];
    const int n = P.p.n, n_words = (n + 63) >> 6;
    const float* X1 = A.X1 + 3 * (size_t)P.corr0;
    const float* X2 = A.X2 + 3 * (size_t)P.corr0;
    float P1[9], P2[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int idx = A.triples[3 * (size_t)g + i];
#pragma unroll
        for (int r = 0; r < 3; r++) { P1[3 * i + r] = X1[3 * (size_t)idx + r]; P2[3 * i + r] = X2[3 * (size_t)idx + r]; }
    }
    msorb::Sim3Transform T;
    msorb::sim3_compute(P1, P2, P.p.fix_scale != 0, T);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long* mask = A.mask + P.mask0 + (unsigned long long)(g - P.hyp0) * n_words;
    int count = 0;
    for (int base = 0; base < n; base += kThreads) {   // uniform trip count: every lane reaches the ballot
        const int i = base + (int)threadIdx.x;
        bool in = false;
        if (i < n) {
            const size_t c = (size_t)P.corr0 + i;
            in = msorb::sim3_is_inlier(T, P.p.cam1, P.p.cam2, X1 + 3 * (size_t)i, X2 + 3 * (size_t)i, A.max_err1[c], A.max_err2[c]);
        }
        const unsigned long long word = __ballot(in);
        count += __popcll(word);
        const int w = (base >> 6) + wave;
        if (lane == 0 && w < n_words) mask[w] = word;
    }
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = wave_count[0];
        for (int w = 1; w < kWaves; w++) total += wave_count[w];
        A.counts[g] = total;
        Sim3Record& r = A.rec[g];
        r.s = T.s;
        for (int k = 0; k < 9; k++) r.R[k] = T.R[k];
        for (int k = 0; k < 3; k++) r.t[k] = T.t[k];
    }
}

__global__ __launch_bounds__(64) void sim3_select_kernel(const Sim3Args A) {
    __shared__ int chunk[kSelectChunk];
    const Sim3ProblemDev P = A.prob[blockIdx.x];
    const int H = P.p.n_hyp, n_words = (P.p.n + 63) >> 6;
    const int* counts = A.counts + P.hyp0;
    // the rule is a fold: a chunk continues from the best the chunks before it left
    msorb::Sim3Selection sel{-1, 0, H, P.p.best_inliers_in};
    for (int base = 0; base < H && !sel.converged; base += kSelectChunk) {
        const int m = min(kSelectChunk, H - base);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += 64) chunk[i] = counts[base + i];
        __syncthreads();
        msorb::sim3_select_continue(sel, chunk, m, base, P.p.min_inliers);   // every lane, on the same data
    }
    unsigned long long* out = A.wmask + P.wmask0;
    const unsigned long long* src = sel.winner >= 0 ? A.mask + P.mask0 + (unsigned long long)sel.winner * n_words : nullptr;
    for (int w = threadIdx.x; w < n_words; w += 64) out[w] = src ? src[w] : 0ull;
    if (threadIdx.x == 0) {
        msorb_sim3_result& R = A.result[blockIdx.x];
        R.winner = sel.winner;
        R.converged = sel.converged;
        R.consumed = sel.consumed;
        Sim3Record r{};
        if (sel.winner >= 0) r = A.rec[P.hyp0 + sel.winner];
        R.n_inliers = sel.winner >= 0 ? counts[sel.winner] : 0;
        R.s = r.s;
        for (int k = 0; k < 9; k++) R.R[k] = r.R[k];
        for (int k = 0; k < 3; k++) R.t[k] = r.t[k];
        // mT12i (:475-479): setIdentity, sR, mt12i
        for (int row = 0; row < 3; row++) {
            for (int c = 0; c < 3; c++) R.T12[4 * row + c] = sel.winner >= 0 ? msorb::np_mul(r.s, r.R[3 * row + c]) : 0.0f;
            R.T12[4 * row + 3] = r.t[row];
        }
        R.T12[12] = 0.0f; R.T12[13] = 0.0f; R.T12[14] = 0.0f; R.T12[15] = sel.winner >= 0 ? 1.0f : 0.0f;
    }
}

int invalid(const char* what) {
    set_last_error(std::string("sim3_ransac_batch: ") + what);
    return MSORB_E_INVALID;
}

}  // namespace

extern "C" int msorb_sim3_ransac_batch(int device, int n_problems, const msorb_sim3_problem* problems, const int* corr_offset,
                                       const int* hyp_offset, const float* X1, const float* X2, const float* max_err1,
                                       const float* max_err2, const int* triples, uint8_t* inlier_out, int* counts_out,
                                       msorb_sim3_result* results, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (n_problems < 0) return invalid("n_problems < 0");
    if (n_problems == 0) return MSORB_OK;
    if (!problems || !corr_offset || !hyp_offset || !X1 || !X2 || !max_err1 || !max_err2 || !triples || !inlier_out || !results)
        return invalid("a required array is null");
    if (corr_offset[0] != 0 || hyp_offset[0] != 0) return invalid("corr_offset[0] and hyp_offset[0] must be 0");
    size_t mask_words = 0, wmask_words = 0;
    for (int i = 0; i < n_problems; i++) {
        const msorb_sim3_problem& p = problems[i];
        if (p.n < 3) return invalid("a problem has fewer than 3 correspondences");
        if (p.n_hyp < 1) return invalid("a problem has no hypothesis");
        if (corr_offset[i + 1] - corr_offset[i] != p.n || hyp_offset[i + 1] - hyp_offset[i] != p.n_hyp)
            return invalid("the offsets do not match the problems' n / n_hyp");
        for (int h = hyp_offset[i]; h < hyp_offset[i + 1]; h++) {
            const int a = triples[3 * (size_t)h], b = triples[3 * (size_t)h + 1], c = triples[3 * (size_t)h + 2];
            if (a < 0 || b < 0 || c < 0 || a >= p.n || b >= p.n || c >= p.n) return invalid("a triple index is out of range");
            if (a == b || a == c || b == c) return invalid("a triple repeats an index");
        }
        const size_t nw = ((size_t)p.n + 63) / 64;
        mask_words += nw * (size_t)p.n_hyp;
        wmask_words += nw;
    }
    if (int rc = msorb::require_device(device)) return rc;
    const size_t total_n = (size_t)corr_offset[n_problems], total_h = (size_t)hyp_offset[n_problems];
    // up: [problems | hyp_problem | triples | X1 | X2 | max_err1 | max_err2]; down: [results | winners' masks | counts]; then the
    // device-only records and masks of all hypotheses
    const size_t o_prob = 0, o_hp = up16((size_t)n_problems * sizeof(Sim3ProblemDev)), o_tr = o_hp + up16(total_h * 4);
    const size_t o_x1 = o_tr + up16(total_h * 12), o_x2 = o_x1 + up16(total_n * 12), o_e1 = o_x2 + up16(total_n * 12);
    const size_t o_e2 = o_e1 + up16(total_n * 4), in_bytes = o_e2 + up16(total_n * 4);
    const size_t o_res = in_bytes, o_wm = o_res + up16((size_t)n_problems * sizeof(msorb_sim3_result)), o_cnt = o_wm + up16(wmask_words * 8);
    const size_t pin_bytes = o_cnt + up16(total_h * 4);
    const size_t o_rec = pin_bytes, o_mask = o_rec + up16(total_h * sizeof(Sim3Record)), dev_bytes = o_mask + up16(mask_words * 8);
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(device, dev_bytes, pin_bytes)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    Sim3ProblemDev* hp = reinterpret_cast<Sim3ProblemDev*>(h + o_prob);
    int* hyp_problem = reinterpret_cast<int*>(h + o_hp);
    size_t m0 = 0, w0 = 0;
    for (int i = 0; i < n_problems; i++) {
        hp[i].p = problems[i];
        hp[i].corr0 = corr_offset[i];
        hp[i].hyp0 = hyp_offset[i];
        hp[i].mask0 = m0;
        hp[i].wmask0 = w0;
        const size_t nw = ((size_t)problems[i].n + 63) / 64;
        m0 += nw * (size_t)problems[i].n_hyp;
        w0 += nw;
        for (int g = hyp_offset[i]; g < hyp_offset[i + 1]; g++) hyp_problem[g] = i;
    }
    std::memcpy(h + o_tr, triples, total_h * 12);
    std::memcpy(h + o_x1, X1, total_n * 12);
    std::memcpy(h + o_x2, X2, total_n * 12);
    std::memcpy(h + o_e1, max_err1, total_n * 4);
    std::memcpy(h + o_e2, max_err2, total_n * 4);
    Sim3Args A{};
    A.prob = reinterpret_cast<const Sim3ProblemDev*>(d + o_prob);
    A.hyp_problem = reinterpret_cast<const int*>(d + o_hp);
    A.triples = reinterpret_cast<const int*>(d + o_tr);
    A.X1 = reinterpret_cast<const float*>(d + o_x1);
    A.X2 = reinterpret_cast<const float*>(d + o_x2);
    A.max_err1 = reinterpret_cast<const float*>(d + o_e1);
    A.max_err2 = reinterpret_cast<const float*>(d + o_e2);
    A.result = reinterpret_cast<msorb_sim3_result*>(d + o_res);
    A.wmask = reinterpret_cast<unsigned long long*>(d + o_wm);
    A.counts = reinterpret_cast<int*>(d + o_cnt);
    A.rec = reinterpret_cast<Sim3Record*>(d + o_rec);
    A.mask = reinterpret_cast<unsigned long long*>(d + o_mask);
    hipStream_t s = scr.s;
    hipError_t e = msorb::small_copy(d, h, in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[0], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sim3_hypotheses_kernel, dim3((unsigned)total_h), dim3(kThreads), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sim3_select_kernel, dim3(n_problems), dim3(64), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[1], s);
    if (e == hipSuccess) e = msorb::small_copy(h + o_res, d + o_res, pin_bytes - o_res, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && elapsed_ms) e = hipEventElapsedTime(elapsed_ms, scr.ev[0], scr.ev[1]);
    if (e != hipSuccess) {
        set_last_error(std::string("sim3_ransac_batch: ") + hipGetErrorString(e));
        scr.release();
        return MSORB_E_HIP;
    }
    std::memcpy(results, h + o_res, (size_t)n_problems * sizeof(msorb_sim3_result));
    if (counts_out) std::memcpy(counts_out, h + o_cnt, total_h * 4);
    const unsigned long long* wm = reinterpret_cast<const unsigned long long*>(h + o_wm);
    for (int i = 0; i < n_problems; i++)
        for (int k = 0; k < problems[i].n; k++)
            inlier_out[(size_t)corr_offset[i] + k] = (uint8_t)((wm[hp[i].wmask0 + (size_t)(k >> 6)] >> (k & 63)) & 1);
    return MSORB_OK;
}
