// MLPnPsolver's RANSAC (src/MLPnPsolver.cpp:143-266) with every hypothesis evaluated at once: msorb_mlpnp_ransac_batch.
//
// The random draws of the reference do not depend on the data (:163-183), so the caller hands in the minimal sets of ALL
// iterations and the loop splits into a map and a scan:
//
//   mlpnp_hypotheses_kernel  one wavefront (a workgroup of 64) per (hypothesis, problem).  computePose (:399-701) of the six
//                            correspondences runs cooperatively on the wavefront's MlpnpWork in LDS (mlpnp_device.h): the rows of A
//                            and of J, the 78 sums of A^T A, the 27 of J^T J and J^T r and the row / column updates of each Jacobi
//                            rotation are one item per lane; what is a dependent chain on uniform data (the rotation's c and s, the
//                            3x3 steps, the 6x6 solve) every lane computes.  All sums are in a fixed order, none atomic.  Then
//                            CheckInliers (:305-336): the wavefront walks its problem's correspondences 64 at a time, a step's 64
//                            decisions are one __ballot word of the hypothesis' mask, the count the popcounts of the words.
//   mlpnp_select_kernel      one wavefront per problem: the sequential rule of :212-263 (mlpnp_select.h) over the counts in
//                            hypothesis order, then the winner's record and mask copied into the block the host reads back.
//
// A hypothesis is a latency-bound chain in double (some hundred dependent Jacobi rotations); what the device offers is that the
// hypotheses of all problems are resident at once, about 5 KB of LDS and one wavefront each.  One upload, two launches, one
// read-back on the calling thread's scratch.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "mlpnp_device.h"
#include "mlpnp_select.h"

namespace msorb {
hipError_t small_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);   // orb_kernels.hip
}
using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;

namespace {

constexpr int kSelectChunk = 1024;   // counts the selection stages in LDS at a time

static_assert(sizeof(msorb_mlpnp_problem) == 32 && sizeof(msorb_mlpnp_result) == 176, "the records of include/msorb.h as the Python mirror lays them out");

struct MlpnpProblemDev {
    msorb_mlpnp_problem p;
    int corr0, hyp0;                    // the problem's first correspondence / hypothesis in the flat arrays
    unsigned long long mask0, wmask0;   // its first mask word among all hypotheses' masks / among the winners' masks
};

struct MlpnpArgs {
    const MlpnpProblemDev* prob;
    const int* hyp_problem;   // per hypothesis: its problem
    const int* sets;          // per hypothesis: six correspondence indices of its problem
    const float *p2d, *p3d, *max_err;
    double* pose;             // per hypothesis: R (9, row major), t (3)
    uint8_t* flags;           // per hypothesis
    unsigned long long* mask; // per hypothesis ceil(n / 64) words
    int* counts;              // per hypothesis
    msorb_mlpnp_result* result;
    unsigned long long* wmask;   // per problem ceil(n / 64) words: the winner's mask
};

__global__ __launch_bounds__(64) void mlpnp_hypotheses_kernel(const MlpnpArgs A) {
    __shared__ msorb::MlpnpWork work;
    const int g = blockIdx.x, lane = threadIdx.x;
    const MlpnpProblemDev P = A.prob[A.hyp_problem[g]];
    const int n = P.p.n, n_words = (n + 63) >> 6;
    const float* p2d = A.p2d + 2 * (size_t)P.corr0;
    const float* p3d = A.p3d + 3 * (size_t)P.corr0;
    const float* max_err = A.max_err + (size_t)P.corr0;
    double R[9], t[3];
    const unsigned flags = msorb::mlpnp_compute_pose(work, lane, 64, P.p.cam, p2d, p3d, A.sets + 6 * (size_t)g, R, t);
    unsigned long long* mask = A.mask + P.mask0 + (unsigned long long)(g - P.hyp0) * n_words;
    int count = 0;
    for (int base = 0; base < n; base += 64) {   // uniform trip count: every lane reaches the ballot
        const int i = base + lane;
        bool in = false;
        if (i < n) in = msorb::mlpnp_is_inlier(R, t, P.p.cam, p3d + 3 * (size_t)i, p2d + 2 * (size_t)i, max_err[i]);
        const unsigned long long word = __ballot(in);
        count += __popcll(word);
        if (lane == 0) mask[base >> 6] = word;
    }
    if (lane == 0) {
        A.counts[g] = count;
        A.flags[g] = (uint8_t)flags;
    }
    if (lane < 12) A.pose[12 * (size_t)g + lane] = lane < 9 ? R[lane] : t[lane - 9];
}

__global__ __launch_bounds__(64) void mlpnp_select_kernel(const MlpnpArgs A) {
    __shared__ int chunk[kSelectChunk];
    const MlpnpProblemDev P = A.prob[blockIdx.x];
    const int H = P.p.n_hyp, n_words = (P.p.n + 63) >> 6;
    const int* counts = A.counts + P.hyp0;
    // the rule is a fold: a chunk continues from the best the chunks before it left
    msorb::MlpnpSelection sel{-1, 0, H, P.p.best_inliers_in, -1};
    for (int base = 0; base < H && !sel.converged; base += kSelectChunk) {
        const int m = min(kSelectChunk, H - base);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += 64) chunk[i] = counts[base + i];
        __syncthreads();
        msorb::mlpnp_select_continue(sel, chunk, m, base, P.p.min_inliers);   // every lane, on the same data
    }
    unsigned long long* out = A.wmask + P.wmask0;
    const unsigned long long* src = sel.winner >= 0 ? A.mask + P.mask0 + (unsigned long long)sel.winner * n_words : nullptr;
    for (int w = threadIdx.x; w < n_words; w += 64) out[w] = src ? src[w] : 0ull;
    if (threadIdx.x == 0) {
        msorb_mlpnp_result& R = A.result[blockIdx.x];
        R.winner = sel.winner;
        R.converged = sel.converged;
        R.consumed = sel.consumed;
        R.n_inliers = sel.winner >= 0 ? counts[sel.winner] : 0;
        const double* pose = sel.winner >= 0 ? A.pose + 12 * (size_t)(P.hyp0 + sel.winner) : nullptr;
        for (int k = 0; k < 9; k++) R.R[k] = pose ? pose[k] : 0.0;
        for (int k = 0; k < 3; k++) R.t[k] = pose ? pose[9 + k] : 0.0;
        // mBestTcw / mRefinedTcw (:220-226, :381-388): setIdentity, Rcw and tcw narrowed to float
        for (int row = 0; row < 3; row++) {
            for (int c = 0; c < 3; c++) R.Tcw[4 * row + c] = pose ? (float)pose[3 * row + c] : 0.0f;
            R.Tcw[4 * row + 3] = pose ? (float)pose[9 + row] : 0.0f;
        }
        R.Tcw[12] = 0.0f; R.Tcw[13] = 0.0f; R.Tcw[14] = 0.0f; R.Tcw[15] = pose ? 1.0f : 0.0f;
    }
}

int invalid(const char* what) {
    set_last_error(std::string("mlpnp_ransac_batch: ") + what);
    return MSORB_E_INVALID;
}

}  // namespace

extern "C" int msorb_mlpnp_ransac_batch(int device, int n_problems, const msorb_mlpnp_problem* problems, const int* corr_offset,
                                        const int* hyp_offset, const float* p2d, const float* p3d_w, const float* max_err,
                                        const int* sets, uint8_t* inlier_out, int* counts_out, double* hyp_pose_out,
                                        uint8_t* hyp_flags_out, msorb_mlpnp_result* results, float* elapsed_ms) {
    if (n_problems < 0) return invalid("n_problems < 0");
    if (n_problems == 0) {
        if (elapsed_ms) *elapsed_ms = 0;
        return MSORB_OK;
    }
    if (!problems || !corr_offset || !hyp_offset || !p2d || !p3d_w || !max_err || !sets || !inlier_out || !results)
        return invalid("a required array is null");
    if (corr_offset[0] != 0 || hyp_offset[0] != 0) return invalid("corr_offset[0] and hyp_offset[0] must be 0");
    size_t mask_words = 0, wmask_words = 0;
    for (int i = 0; i < n_problems; i++) {
        const msorb_mlpnp_problem& p = problems[i];
        if (p.n < 6) return invalid("a problem has fewer than 6 correspondences");
        if (p.n_hyp < 1) return invalid("a problem has no hypothesis");
        if (corr_offset[i + 1] - corr_offset[i] != p.n || hyp_offset[i + 1] - hyp_offset[i] != p.n_hyp)
            return invalid("the offsets do not match the problems' n / n_hyp");
        for (int h = hyp_offset[i]; h < hyp_offset[i + 1]; h++) {
            const int* s = sets + 6 * (size_t)h;
            for (int a = 0; a < 6; a++) {
                if (s[a] < 0 || s[a] >= p.n) return invalid("an index of a set is out of range");
                for (int b = 0; b < a; b++)
                    if (s[a] == s[b]) return invalid("a set repeats an index");
            }
        }
        const size_t nw = ((size_t)p.n + 63) / 64;
        mask_words += nw * (size_t)p.n_hyp;
        wmask_words += nw;
    }
    if (int rc = msorb::require_device(device)) return rc;
    if (elapsed_ms) *elapsed_ms = 0;
    const size_t total_n = (size_t)corr_offset[n_problems], total_h = (size_t)hyp_offset[n_problems];
    // up: [problems | hyp_problem | sets | p2d | p3d | max_err]; down: [results | winners' masks | counts | poses | flags]; then the
    // device-only masks of all hypotheses
    const size_t o_prob = 0, o_hp = up16((size_t)n_problems * sizeof(MlpnpProblemDev)), o_set = o_hp + up16(total_h * 4);
    const size_t o_2d = o_set + up16(total_h * 24), o_3d = o_2d + up16(total_n * 8), o_err = o_3d + up16(total_n * 12);
    const size_t in_bytes = o_err + up16(total_n * 4);
    const size_t o_res = in_bytes, o_wm = o_res + up16((size_t)n_problems * sizeof(msorb_mlpnp_result)), o_cnt = o_wm + up16(wmask_words * 8);
    const size_t o_pose = o_cnt + up16(total_h * 4), o_flag = o_pose + up16(total_h * 96), pin_bytes = o_flag + up16(total_h);
    const size_t o_mask = pin_bytes, dev_bytes = o_mask + up16(mask_words * 8);
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(device, dev_bytes, pin_bytes)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    MlpnpProblemDev* hp = reinterpret_cast<MlpnpProblemDev*>(h + o_prob);
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
    std::memcpy(h + o_set, sets, total_h * 24);
    std::memcpy(h + o_2d, p2d, total_n * 8);
    std::memcpy(h + o_3d, p3d_w, total_n * 12);
    std::memcpy(h + o_err, max_err, total_n * 4);
    MlpnpArgs A{};
    A.prob = reinterpret_cast<const MlpnpProblemDev*>(d + o_prob);
    A.hyp_problem = reinterpret_cast<const int*>(d + o_hp);
    A.sets = reinterpret_cast<const int*>(d + o_set);
    A.p2d = reinterpret_cast<const float*>(d + o_2d);
    A.p3d = reinterpret_cast<const float*>(d + o_3d);
    A.max_err = reinterpret_cast<const float*>(d + o_err);
    A.result = reinterpret_cast<msorb_mlpnp_result*>(d + o_res);
    A.wmask = reinterpret_cast<unsigned long long*>(d + o_wm);
    A.counts = reinterpret_cast<int*>(d + o_cnt);
    A.pose = reinterpret_cast<double*>(d + o_pose);
    A.flags = d + o_flag;
    A.mask = reinterpret_cast<unsigned long long*>(d + o_mask);
    hipStream_t s = scr.s;
    hipError_t e = msorb::small_copy(d, h, in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[0], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mlpnp_hypotheses_kernel, dim3((unsigned)total_h), dim3(64), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mlpnp_select_kernel, dim3(n_problems), dim3(64), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[1], s);
    if (e == hipSuccess) e = msorb::small_copy(h + o_res, d + o_res, pin_bytes - o_res, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && elapsed_ms) e = hipEventElapsedTime(elapsed_ms, scr.ev[0], scr.ev[1]);
    if (e != hipSuccess) {
        set_last_error(std::string("mlpnp_ransac_batch: ") + hipGetErrorString(e));
        scr.release();
        return MSORB_E_HIP;
    }
    std::memcpy(results, h + o_res, (size_t)n_problems * sizeof(msorb_mlpnp_result));
    if (counts_out) std::memcpy(counts_out, h + o_cnt, total_h * 4);
    if (hyp_pose_out) std::memcpy(hyp_pose_out, h + o_pose, total_h * 96);
    if (hyp_flags_out) std::memcpy(hyp_flags_out, h + o_flag, total_h);
    const unsigned long long* wm = reinterpret_cast<const unsigned long long*>(h + o_wm);
    for (int i = 0; i < n_problems; i++)
        for (int k = 0; k < problems[i].n; k++)
            inlier_out[(size_t)corr_offset[i] + k] = (uint8_t)((wm[hp[i].wmask0 + (size_t)(k >> 6)] >> (k & 63)) & 1);
    return MSORB_OK;
}
