// TwoViewReconstruction::Reconstruct through ms-slam_amd/csrc/two_view_device.h and two_view_select.h on the host, serially (lane 0
// of 1): the yardstick of the device tests and the host side of the latency comparison.  It is the text the kernels compile, driven
// by plain loops in the reference's order; build with -ffp-contract=off.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../ms-slam_amd/csrc/two_view_device.h"
#include "../ms-slam_amd/csrc/two_view_select.h"

namespace tv_host {

struct Result {   // msorb_two_view_result
    int ok, branch, winner_h, winner_f, n_motion, chosen, n_inliers;
    float SH, SF, RH;
    float R[9], t[3];
    float model[9];
    int n_good[8];
    float parallax[8], cosine[8];
    float motion_R[72], motion_t[24];
};
static_assert(sizeof(Result) == 604, "msorb_two_view_result");

struct Problem {
    int n1 = 0, n2 = 0, n_hyp = 0, min_triangulated = 50;
    float cam[4] = {}, sigma = 1.0f, min_parallax = 1.0f;
    double h_ratio = 0.5;
    std::vector<float> keys1, keys2;
    std::vector<int> matches12, sets;
};

struct Answer {
    Result r{};
    std::vector<uint8_t> triangulated, inliers, masks, status;   // [n1], [n], [2 H n], [8 n]
    std::vector<float> p3d, scores;                              // [n1 3], [2 H]
    std::vector<int> counts;                                     // [2 H]
    int n = 0;
};

// Normalize (:737-784) over all keypoints of a frame
inline msorb::TvNorm normalize(const float* keys, int n) {
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

// FindHomography (model 0) or FindFundamental (model 1): every hypothesis' score, count, mask and model
inline void find_model(int model, const Problem& p, const std::vector<float>& m, int n, const msorb::TvNorm& norm1, const msorb::TvNorm& norm2,
                       float* scores, int* counts, uint8_t* masks, float* models) {
    using namespace msorb;
    float T1[9], T2[9];
    tv_norm_matrix(norm1, T1);
    tv_norm_matrix(norm2, T2);
    const float inv_sigma_square = tv_inv_sigma_square(p.sigma);
    TvWork work;
    for (int h = 0; h < p.n_hyp; h++) {
        for (int j = 0; j < 8; j++) {
            const float* q = &m[4 * (size_t)p.sets[8 * (size_t)h + j]];
            float pn[4];
            tv_normalize_point(norm1, q[0], q[1], pn[0], pn[1]);
            tv_normalize_point(norm2, q[2], q[3], pn[2], pn[3]);
            if (model) tv_fill_f_row(work, j, pn);
            else tv_fill_h_rows(work, j, pn);
        }
        float x[9], M[9], Minv[9];
        tv_null_vector(work, 0, 1, model ? 8 : 16, x);
        if (model) tv_fundamental_from_null(x, T1, T2, M);
        else tv_homography_from_null(x, T1, T2, M, Minv);
        float score = 0.0f;
        int count = 0;
        for (int i = 0; i < n; i++) {
            const float* q = &m[4 * (size_t)i];
            float t1, t2;
            const bool in = model ? tv_fundamental_terms(M, q[0], q[1], q[2], q[3], inv_sigma_square, t1, t2)
                                  : tv_homography_terms(M, Minv, q[0], q[1], q[2], q[3], inv_sigma_square, t1, t2);
            score = np_add(score, t1);
            score = np_add(score, t2);
            masks[(size_t)h * n + i] = in;
            count += in;
        }
        scores[h] = score;
        counts[h] = count;
        std::memcpy(models + 9 * (size_t)h, M, sizeof M);
    }
}

// threads: 1, or 2 as the reference runs FindHomography and FindFundamental (:105-110)
inline Answer reconstruct(const Problem& p, int threads = 1) {
    using namespace msorb;
    Answer a;
    std::vector<float> m;
    std::vector<int> first;
    for (int i = 0; i < p.n1; i++)
        if (p.matches12[i] >= 0) {
            const int j = p.matches12[i];
            m.insert(m.end(), {p.keys1[2 * (size_t)i], p.keys1[2 * (size_t)i + 1], p.keys2[2 * (size_t)j], p.keys2[2 * (size_t)j + 1]});
            first.push_back(i);
        }
    const int n = (int)first.size(), H = p.n_hyp;
    a.n = n;
    a.triangulated.assign(p.n1, 0);
    a.p3d.assign(3 * (size_t)p.n1, 0.0f);
    a.inliers.assign(n, 0);
    a.scores.assign(2 * (size_t)H, 0.0f);
    a.counts.assign(2 * (size_t)H, 0);
    a.masks.assign(2 * (size_t)H * n, 0);
    a.status.assign(8 * (size_t)n, 0);
    std::vector<float> models(18 * (size_t)H);
    const TvNorm norm1 = normalize(p.keys1.data(), p.n1), norm2 = normalize(p.keys2.data(), p.n2);
    auto run = [&](int model) {
        find_model(model, p, m, n, norm1, norm2, &a.scores[(size_t)model * H], &a.counts[(size_t)model * H], &a.masks[(size_t)model * H * n],
                   &models[9 * (size_t)model * H]);
    };
    if (threads >= 2) {
        std::thread th(run, 0), tf(run, 1);
        th.join();
        tf.join();
    } else {
        run(0);
        run(1);
    }
    TvFold fold[2] = {{0.0f, -1}, {0.0f, -1}};
    tv_fold_continue(fold[0], &a.scores[0], H, 0);
    tv_fold_continue(fold[1], &a.scores[H], H, 0);
    Result& r = a.r;
    r.branch = tv_branch(fold[0].score, fold[1].score, p.h_ratio, r.RH);
    r.winner_h = fold[0].winner;
    r.winner_f = fold[1].winner;
    r.SH = fold[0].score;
    r.SF = fold[1].score;
    r.chosen = -1;
    const int w = r.branch == kTvHomography ? fold[0].winner : r.branch == kTvFundamental ? fold[1].winner : -1;
    if (w < 0) return a;
    const size_t g = r.branch == kTvHomography ? (size_t)w : (size_t)H + w;
    std::memcpy(r.model, &models[9 * g], sizeof r.model);
    std::memcpy(a.inliers.data(), &a.masks[g * n], n);
    r.n_inliers = a.counts[g];
    if (r.branch == kTvHomography) r.n_motion = tv_motions_from_h(r.model, p.cam, r.motion_R, r.motion_t) ? 8 : 0;
    else { tv_motions_from_f(r.model, p.cam, r.motion_R, r.motion_t); r.n_motion = 4; }
    if (r.n_motion == 0) { std::memset(r.motion_R, 0, sizeof r.motion_R); std::memset(r.motion_t, 0, sizeof r.motion_t); }
    std::vector<float> pts(24 * (size_t)n, 0.0f);
    for (int mh = 0; mh < r.n_motion; mh++) {
        TvPose P;
        tv_pose_setup(r.motion_R + 9 * mh, r.motion_t + 3 * mh, p.cam, p.sigma, P);
        std::vector<float> cosines;
        for (int i = 0; i < n; i++) {
            if (!a.inliers[i]) continue;
            float X[3], c;
            const int st = tv_check_point(P, m[4 * (size_t)i], m[4 * (size_t)i + 1], m[4 * (size_t)i + 2], m[4 * (size_t)i + 3], X, c);
            a.status[(size_t)mh * n + i] = (uint8_t)st;
            if (st == kTvRejected) continue;
            cosines.push_back(c);
            std::memcpy(&pts[3 * ((size_t)mh * n + i)], X, 12);
        }
        r.n_good[mh] = (int)cosines.size();
        if (!cosines.empty()) {
            std::sort(cosines.begin(), cosines.end());
            r.cosine[mh] = cosines[std::min<size_t>(50, cosines.size() - 1)];
            r.parallax[mh] = (float)((double)(std::acos(r.cosine[mh]) * 180.0f) / 3.1415926535897932384626433832795);
        }
    }
    if (r.n_motion == 4) r.chosen = tv_final_f(r.n_good, r.parallax, r.n_inliers, p.min_parallax, p.min_triangulated);
    if (r.n_motion == 8) r.chosen = tv_final_h(r.n_good, r.parallax, r.n_inliers, p.min_parallax, p.min_triangulated);
    r.ok = r.chosen >= 0;
    if (r.ok) {
        std::memcpy(r.R, r.motion_R + 9 * r.chosen, sizeof r.R);
        std::memcpy(r.t, r.motion_t + 3 * r.chosen, sizeof r.t);
        for (int i = 0; i < n; i++) {
            const int st = a.status[(size_t)r.chosen * n + i];
            if (st == kTvRejected) continue;
            std::memcpy(&a.p3d[3 * (size_t)first[i]], &pts[3 * ((size_t)r.chosen * n + i)], 12);
            a.triangulated[first[i]] = st == kTvGood;
        }
    }
    return a;
}

}  // namespace tv_host
