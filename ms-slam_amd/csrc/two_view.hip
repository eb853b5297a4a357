// TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc:41-129) for a pinhole camera on the device, every RANSAC
// hypothesis of both models at once: msorb_two_view_reconstruct.
//
// The reference draws all minimal sets before its loops (:79-98) and has no early exit, so the caller hands the sets in and the work
// splits into a map, a scan and a second map:
//
//   two_view_hypotheses_kernel  one workgroup of 256 threads per (model, hypothesis).  The 8 (F) or 16 (H) rows of the design matrix
//                               go to LDS and the workgroup runs the one-sided Jacobi of two_view_device.h on them: the rotation's
//                               c, s on every thread from LDS, row k of A / V on thread k, a barrier between reading and writing.
//                               (The redundant per-thread form of sim3.hip would hold 144 + 81 floats under dynamic column indices,
//                               which is scratch; through LDS the kernel needs none.)  Every thread then forms the model (rank-2 step,
//                               denormalisation, inverse) redundantly in registers.  Thread t takes the matches t, t + 256, ...:
//                               a wavefront's 64 decisions are one __ballot word of the mask; the two score terms of each match go
//                               to LDS and thread 0 adds the 512 terms of a pass left to right, in match order, to the score.
//   two_view_motion_kernel      one wavefront: the two folds over the scores, Reconstruct's branch, the 8 or 4 motion hypotheses of
//                               the winning model, the winner's mask copied to where the host reads it.
//   two_view_check_kernel       one workgroup per motion hypothesis: CheckRT over the winner's inliers, one match per thread and
//                               pass; nGood from popcounts added in ascending wavefront order; the accepted cosine of rank
//                               min(50, nGood - 1) found by counting, for every accepted value, the accepted values before it in
//                               (value, match index) order, which is the element std::sort would leave at that index.
//
// One upload, three launches, one read-back on the calling thread's scratch; no atomics.  acos and the closing rule run on the host
// with the host's libm (two_view_select.h), as the reference's do.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "two_view_device.h"
#include "two_view_select.h"

namespace msorb {
hipError_t small_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);   // orb_kernels.hip
}
using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kFoldChunk = 1024;     // scores the fold stages in LDS at a time
constexpr int kRankChunk = 2048;     // cosines the rank count stages in LDS at a time
constexpr int kMaxMatches = 32768;   // the matcher's keypoints per frame

static_assert(sizeof(msorb_two_view_result) == 604, "the record of include/msorb.h as the Python mirror lays it out");

struct TvMotionRecord {   // what the motion kernel leaves for the check kernel and the host
    int branch, winner_h, winner_f, n_motion, n_inliers;
    float SH, SF, RH;
    float model[9];
    float R[72], t[24];
};

struct TvArgs {
    int n, n_hyp, n_words;
    msorb::TvNorm norm1, norm2;
    float cam[4];
    float sigma;
    double h_ratio;
    const float* m;           // per match u1, v1, u2, v2
    const int* sets;          // per hypothesis eight match indices
    float* score;             // [2 n_hyp]: H then F
    int* count;               // [2 n_hyp]
    float* model;             // [2 n_hyp][9]
    unsigned long long* mask; // [2 n_hyp][n_words]
    TvMotionRecord* motion;
    unsigned long long* wmask;   // [n_words] the winner's
    int* n_good;              // [8]
    float* cosine;            // [8]
    uint8_t* status;          // [8][n]
    float* p3d;               // [8][n][3]
    float* cosv;              // [8][n] accepted cosines (3.0f elsewhere)
};

__global__ __launch_bounds__(kThreads) void two_view_hypotheses_kernel(const TvArgs A) {
    __shared__ msorb::TvWork work;
    __shared__ __align__(16) float terms[2 * kThreads];
    __shared__ int wave_count[kWaves];
    const int g = blockIdx.x, tid = threadIdx.x;
    const bool is_f = g >= A.n_hyp;
    const int n = A.n;
    if (tid < 8) {
        const int idx = A.sets[8 * (size_t)(is_f ? g - A.n_hyp : g) + tid];
        const float* m = A.m + 4 * (size_t)idx;
        float pn[4];
        msorb::tv_normalize_point(A.norm1, m[0], m[1], pn[0], pn[1]);
        msorb::tv_normalize_point(A.norm2, m[2], m[3], pn[2], pn[3]);
        if (is_f) msorb::tv_fill_f_row(work, tid, pn);
        else msorb::tv_fill_h_rows(work, tid, pn);
    }
    __syncthreads();
    float x[9];
    msorb::tv_null_vector(work, tid, kThreads, is_f ? 8 : 16, x);
    float T1[9], T2[9], M[9], Minv[9];
    msorb::tv_norm_matrix(A.norm1, T1);
    msorb::tv_norm_matrix(A.norm2, T2);
    if (is_f) msorb::tv_fundamental_from_null(x, T1, T2, M);
    else msorb::tv_homography_from_null(x, T1, T2, M, Minv);
    const float inv_sigma_square = msorb::tv_inv_sigma_square(A.sigma);
    const int lane = tid & 63, wave = tid >> 6;
    unsigned long long* mask = A.mask + (size_t)g * A.n_words;
    int count = 0;
    float score = 0.0f;
    for (int base = 0; base < n; base += kThreads) {   // uniform trip count: every lane reaches the ballot and the barriers
        const int i = base + tid;
        bool in = false;
        float t1 = 0.0f, t2 = 0.0f;
        if (i < n) {
            const float* m = A.m + 4 * (size_t)i;
            in = is_f ? msorb::tv_fundamental_terms(M, m[0], m[1], m[2], m[3], inv_sigma_square, t1, t2)
                      : msorb::tv_homography_terms(M, Minv, m[0], m[1], m[2], m[3], inv_sigma_square, t1, t2);
        }
        const unsigned long long word = __ballot(in);
        count += __popcll(word);
        const int w = (base >> 6) + wave;
        if (lane == 0 && w < A.n_words) mask[w] = word;
        terms[2 * tid] = t1;
        terms[2 * tid + 1] = t2;
        __syncthreads();
        if (tid == 0) {
            // the reference's chain: serial by definition.  All 512 slots are added: those past the last match hold +0.0f, which
            // adds exactly, so the trip count is fixed and the loads (four terms each) run ahead of the dependent additions
            const float4* t4 = reinterpret_cast<const float4*>(terms);
#pragma unroll 8
            for (int k = 0; k < 2 * kThreads / 4; k++) {
                const float4 v = t4[k];
                score = msorb::np_add(msorb::np_add(msorb::np_add(msorb::np_add(score, v.x), v.y), v.z), v.w);
            }
        }
        __syncthreads();
    }
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (tid == 0) {
        int total = wave_count[0];
        for (int w = 1; w < kWaves; w++) total += wave_count[w];
        A.count[g] = total;
        A.score[g] = score;
    }
    if (tid < 9) A.model[9 * (size_t)g + tid] = M[tid];
}

__global__ __launch_bounds__(64) void two_view_motion_kernel(const TvArgs A) {
    __shared__ float chunk[kFoldChunk];
    const int H = A.n_hyp;
    msorb::TvFold fold[2] = {{0.0f, -1}, {0.0f, -1}};
    for (int model = 0; model < 2; model++)
        for (int base = 0; base < H; base += kFoldChunk) {
            const int m = min(kFoldChunk, H - base);
            __syncthreads();
            for (int i = threadIdx.x; i < m; i += 64) chunk[i] = A.score[(size_t)model * H + base + i];
            __syncthreads();
            msorb::tv_fold_continue(fold[model], chunk, m, base);   // every lane, on the same data
        }
    float RH;
    const int branch = msorb::tv_branch(fold[0].score, fold[1].score, A.h_ratio, RH);
    const int winner = branch == msorb::kTvHomography ? fold[0].winner : branch == msorb::kTvFundamental ? fold[1].winner : -1;
    const int g = winner < 0 ? -1 : branch == msorb::kTvHomography ? winner : H + winner;
    float M[9], R[72], t[24];
    for (int k = 0; k < 72; k++) R[k] = 0.0f;
    for (int k = 0; k < 24; k++) t[k] = 0.0f;
    for (int k = 0; k < 9; k++) M[k] = g >= 0 ? A.model[9 * (size_t)g + k] : 0.0f;
    int n_motion = 0;
    if (g >= 0 && branch == msorb::kTvHomography) n_motion = msorb::tv_motions_from_h(M, A.cam, R, t) ? 8 : 0;
    if (g >= 0 && branch == msorb::kTvFundamental) { msorb::tv_motions_from_f(M, A.cam, R, t); n_motion = 4; }
    for (int w = threadIdx.x; w < A.n_words; w += 64) A.wmask[w] = g >= 0 ? A.mask[(size_t)g * A.n_words + w] : 0ull;
    if (threadIdx.x == 0) {
        TvMotionRecord& r = *A.motion;
        r.branch = branch;
        r.winner_h = fold[0].winner;
        r.winner_f = fold[1].winner;
        r.n_motion = n_motion;
        r.n_inliers = g >= 0 ? A.count[g] : 0;
        r.SH = fold[0].score;
        r.SF = fold[1].score;
        r.RH = RH;
        for (int k = 0; k < 9; k++) r.model[k] = M[k];
        for (int k = 0; k < 72; k++) r.R[k] = R[k];
        for (int k = 0; k < 24; k++) r.t[k] = t[k];
    }
    if (threadIdx.x < 8) { A.n_good[threadIdx.x] = 0; A.cosine[threadIdx.x] = 0.0f; }
}

__global__ __launch_bounds__(kThreads) void two_view_check_kernel(const TvArgs A) {
    __shared__ float chunk[kRankChunk];
    __shared__ int wave_count[kWaves];
    __shared__ int total_s;
    const int mh = blockIdx.x, tid = threadIdx.x, n = A.n;
    const TvMotionRecord& rec = *A.motion;
    if (mh >= rec.n_motion) return;   // the whole workgroup
    msorb::TvPose P;
    msorb::tv_pose_setup(rec.R + 9 * mh, rec.t + 3 * mh, A.cam, A.sigma, P);
    uint8_t* status = A.status + (size_t)mh * n;
    float* p3d = A.p3d + 3 * (size_t)mh * n;
    float* cosv = A.cosv + (size_t)mh * n;
    int count = 0;
    for (int base = 0; base < n; base += kThreads) {
        const int i = base + tid;
        int st = msorb::kTvRejected;
        float X[3] = {0.0f, 0.0f, 0.0f}, c = 3.0f;
        if (i < n && ((A.wmask[i >> 6] >> (i & 63)) & 1ull)) {
            const float* m = A.m + 4 * (size_t)i;
            float cc = 0.0f;
            st = msorb::tv_check_point(P, m[0], m[1], m[2], m[3], X, cc);
            if (st != msorb::kTvRejected) c = cc;
            else { X[0] = 0.0f; X[1] = 0.0f; X[2] = 0.0f; }
        }
        count += __popcll(__ballot(st != msorb::kTvRejected));
        if (i < n) {
            status[i] = (uint8_t)st;
            cosv[i] = c;
            p3d[3 * (size_t)i] = X[0]; p3d[3 * (size_t)i + 1] = X[1]; p3d[3 * (size_t)i + 2] = X[2];
        }
    }
    if ((tid & 63) == 0) wave_count[tid >> 6] = count;
    __syncthreads();   // also orders this workgroup's cosv stores before its loads below
    if (tid == 0) {
        int total = wave_count[0];
        for (int w = 1; w < kWaves; w++) total += wave_count[w];
        total_s = total;
        A.n_good[mh] = total;
    }
    __syncthreads();
    const int n_good = total_s;
    if (n_good == 0) return;
    const int want = min(50, n_good - 1);
    for (int base = 0; base < n; base += kThreads) {
        const int i = base + tid;
        const float ci = i < n ? cosv[i] : 3.0f;
        const bool mine = ci != 3.0f;
        int rank = 0;
        for (int cb = 0; cb < n; cb += kRankChunk) {
            const int m = min(kRankChunk, n - cb);
            __syncthreads();
            for (int k = tid; k < m; k += kThreads) chunk[k] = cosv[cb + k];
            __syncthreads();
            if (mine)
                for (int k = 0; k < m; k++) {
                    const float cj = chunk[k];
                    rank += (cj < ci || (cj == ci && cb + k < i)) ? 1 : 0;   // 3.0f, the mark of a match that was not accepted, is never below
                }
        }
        if (mine && rank == want) A.cosine[mh] = ci;
    }
}

int invalid(const char* what) {
    set_last_error(std::string("two_view_reconstruct: ") + what);
    return MSORB_E_INVALID;
}

// Normalize (:737-784) over ALL keypoints of a frame: four sequential float sums
msorb::TvNorm normalize(const float* keys, int n) {
    using namespace msorb;
    float mean_x = 0.0f, mean_y = 0.0f;
    for (int i = 0; i < n; i++) { mean_x = np_add(mean_x, keys[2 * (size_t)i]); mean_y = np_add(mean_y, keys[2 * (size_t)i + 1]); }
    mean_x = np_div(mean_x, (float)n);
    mean_y = np_div(mean_y, (float)n);
    float dev_x = 0.0f, dev_y = 0.0f;
    for (int i = 0; i < n; i++) {
        dev_x = np_add(dev_x, np_abs(np_sub(keys[2 * (size_t)i], mean_x)));
        dev_y = np_add(dev_y, np_abs(np_sub(keys[2 * (size_t)i + 1], mean_y)));
    }
    dev_x = np_div(dev_x, (float)n);
    dev_y = np_div(dev_y, (float)n);
    return TvNorm{mean_x, mean_y, (float)np_ddiv(1.0, (double)dev_x), (float)np_ddiv(1.0, (double)dev_y)};
}

}  // namespace

extern "C" int msorb_two_view_reconstruct(int device, int n1, const float* keys1, int n2, const float* keys2, const int* matches12,
                                          int n_hyp, const int* sets, float fx, float fy, float cx, float cy, float sigma,
                                          double h_ratio, float min_parallax, int min_triangulated, msorb_two_view_result* result,
                                          uint8_t* triangulated, float* p3d, uint8_t* inlier_out, float* hyp_score_out,
                                          int* hyp_count_out, uint8_t* hyp_mask_out, float* elapsed_ms) {
    if (n1 < 0 || n2 < 0) return invalid("n1 or n2 < 0");
    if (!keys1 || !keys2 || !matches12 || !sets || !result || !triangulated || !p3d || !inlier_out) return invalid("a required array is null");
    if (n_hyp < 1) return invalid("n_hyp < 1");
    int n = 0;
    for (int i = 0; i < n1; i++) {
        if (matches12[i] >= n2) return invalid("a match index is >= n2");
        if (matches12[i] >= 0) n++;
    }
    if (n < 8) return invalid("fewer than 8 matches");
    for (int h = 0; h < n_hyp; h++) {
        const int* s = sets + 8 * (size_t)h;
        for (int a = 0; a < 8; a++) {
            if (s[a] < 0 || s[a] >= n) return invalid("a set index is out of range");
            for (int b = 0; b < a; b++)
                if (s[a] == s[b]) return invalid("a set repeats an index");
        }
    }
    if (n > kMaxMatches) {
        set_last_error("two_view_reconstruct: more than 32768 matches");
        return MSORB_E_CAPACITY;
    }
    if (int rc = msorb::require_device(device)) return rc;
    const size_t N = (size_t)n, H2 = 2 * (size_t)n_hyp, nw = (N + 63) / 64;
    // up: [matches | sets]; down: [motion | n_good | cosine | winner's mask | scores | counts | status | points | (all masks)];
    // device only: models, all masks (when they are not read back), accepted cosines
    const size_t o_m = 0, o_sets = o_m + up16(N * 16), in_bytes = o_sets + up16((size_t)n_hyp * 32);
    const size_t o_mot = in_bytes, o_ng = o_mot + up16(sizeof(TvMotionRecord)), o_cos = o_ng + up16(32), o_wm = o_cos + up16(32);
    const size_t o_sc = o_wm + up16(nw * 8), o_cnt = o_sc + up16(H2 * 4), o_st = o_cnt + up16(H2 * 4), o_p3 = o_st + up16(8 * N);
    const size_t o_mask = o_p3 + up16(8 * N * 12);
    const size_t down_end = hyp_mask_out ? o_mask + up16(H2 * nw * 8) : o_mask;
    const size_t o_model = o_mask + up16(H2 * nw * 8), o_cosv = o_model + up16(H2 * 36), dev_bytes = o_cosv + up16(8 * N * 4);
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(device, dev_bytes, down_end)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    float* hm = reinterpret_cast<float*>(h + o_m);
    for (int i = 0, k = 0; i < n1; i++)
        if (matches12[i] >= 0) {
            hm[4 * (size_t)k] = keys1[2 * (size_t)i];
            hm[4 * (size_t)k + 1] = keys1[2 * (size_t)i + 1];
            hm[4 * (size_t)k + 2] = keys2[2 * (size_t)matches12[i]];
            hm[4 * (size_t)k + 3] = keys2[2 * (size_t)matches12[i] + 1];
            k++;
        }
    std::memcpy(h + o_sets, sets, (size_t)n_hyp * 32);
    TvArgs A{};
    A.n = n; A.n_hyp = n_hyp; A.n_words = (int)nw;
    A.norm1 = normalize(keys1, n1);
    A.norm2 = normalize(keys2, n2);
    A.cam[0] = fx; A.cam[1] = fy; A.cam[2] = cx; A.cam[3] = cy;
    A.sigma = sigma;
    A.h_ratio = h_ratio;
    A.m = reinterpret_cast<const float*>(d + o_m);
    A.sets = reinterpret_cast<const int*>(d + o_sets);
    A.motion = reinterpret_cast<TvMotionRecord*>(d + o_mot);
    A.n_good = reinterpret_cast<int*>(d + o_ng);
    A.cosine = reinterpret_cast<float*>(d + o_cos);
    A.wmask = reinterpret_cast<unsigned long long*>(d + o_wm);
    A.score = reinterpret_cast<float*>(d + o_sc);
    A.count = reinterpret_cast<int*>(d + o_cnt);
    A.status = d + o_st;
    A.p3d = reinterpret_cast<float*>(d + o_p3);
    A.mask = reinterpret_cast<unsigned long long*>(d + o_mask);
    A.model = reinterpret_cast<float*>(d + o_model);
    A.cosv = reinterpret_cast<float*>(d + o_cosv);
    hipStream_t s = scr.s;
    hipError_t e = msorb::small_copy(d, h, in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[0], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(two_view_hypotheses_kernel, dim3((unsigned)H2), dim3(kThreads), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(two_view_motion_kernel, dim3(1), dim3(64), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(two_view_check_kernel, dim3(8), dim3(kThreads), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[1], s);
    if (e == hipSuccess) e = msorb::small_copy(h + o_mot, d + o_mot, down_end - o_mot, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    float ms = 0.0f;
    if (e == hipSuccess && elapsed_ms) e = hipEventElapsedTime(&ms, scr.ev[0], scr.ev[1]);
    if (e != hipSuccess) {
        set_last_error(std::string("two_view_reconstruct: ") + hipGetErrorString(e));
        scr.release();
        return MSORB_E_HIP;
    }
    if (elapsed_ms) *elapsed_ms = ms;
    const TvMotionRecord& rec = *reinterpret_cast<const TvMotionRecord*>(h + o_mot);
    const int* n_good = reinterpret_cast<const int*>(h + o_ng);
    const float* cosine = reinterpret_cast<const float*>(h + o_cos);
    msorb_two_view_result r{};
    r.branch = rec.branch; r.winner_h = rec.winner_h; r.winner_f = rec.winner_f; r.n_motion = rec.n_motion; r.n_inliers = rec.n_inliers;
    r.SH = rec.SH; r.SF = rec.SF; r.RH = rec.RH;
    std::memcpy(r.model, rec.model, sizeof r.model);
    std::memcpy(r.motion_R, rec.R, sizeof r.motion_R);
    std::memcpy(r.motion_t, rec.t, sizeof r.motion_t);
    for (int i = 0; i < 8; i++) {
        r.n_good[i] = i < rec.n_motion ? n_good[i] : 0;
        r.cosine[i] = i < rec.n_motion ? cosine[i] : 0.0f;
        // parallax = acos(vCosParallax[idx]) * 180 / CV_PI (:895): acos of a float under `using namespace std` is the float overload,
        // * 180 a float product, / CV_PI a double division narrowed to the float parallax
        r.parallax[i] = r.n_good[i] > 0 ? (float)((double)(std::acos(r.cosine[i]) * 180.0f) / 3.1415926535897932384626433832795) : 0.0f;
    }
    r.chosen = -1;
    if (rec.n_motion == 4) r.chosen = msorb::tv_final_f(r.n_good, r.parallax, rec.n_inliers, min_parallax, min_triangulated);
    if (rec.n_motion == 8) r.chosen = msorb::tv_final_h(r.n_good, r.parallax, rec.n_inliers, min_parallax, min_triangulated);
    r.ok = r.chosen >= 0;
    if (r.ok) {
        std::memcpy(r.R, rec.R + 9 * r.chosen, sizeof r.R);
        std::memcpy(r.t, rec.t + 3 * r.chosen, sizeof r.t);
    }
    *result = r;
    std::memset(triangulated, 0, (size_t)n1);
    std::memset(p3d, 0, (size_t)n1 * 12);
    const unsigned long long* wm = reinterpret_cast<const unsigned long long*>(h + o_wm);
    const uint8_t* st = h + o_st + (size_t)(r.ok ? r.chosen : 0) * N;
    const float* pts = reinterpret_cast<const float*>(h + o_p3) + 3 * (size_t)(r.ok ? r.chosen : 0) * N;
    for (int i = 0, k = 0; i < n1; i++)
        if (matches12[i] >= 0) {
            inlier_out[k] = (uint8_t)((wm[k >> 6] >> (k & 63)) & 1);
            if (r.ok && st[k] != msorb::kTvRejected) {   // vP3D / vbGood are indexed by the keypoint of frame 1 (:883, :887)
                std::memcpy(p3d + 3 * (size_t)i, pts + 3 * (size_t)k, 12);
                triangulated[i] = st[k] == msorb::kTvGood;
            }
            k++;
        }
    if (hyp_score_out) std::memcpy(hyp_score_out, h + o_sc, H2 * 4);
    if (hyp_count_out) std::memcpy(hyp_count_out, h + o_cnt, H2 * 4);
    if (hyp_mask_out) {
        const unsigned long long* am = reinterpret_cast<const unsigned long long*>(h + o_mask);
        for (size_t g = 0; g < H2; g++)
            for (size_t k = 0; k < N; k++) hyp_mask_out[g * N + k] = (uint8_t)((am[g * nw + (k >> 6)] >> (k & 63)) & 1);
    }
    return MSORB_OK;
}
