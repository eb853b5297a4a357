// ORB_SLAM3::msorb_host::Sim3Solver (ms-slam_amd/host/Sim3Solver_device.h) compiled against the stand-ins of tests/slam_stub and
// driven the way LoopClosing::DetectCommonRegionsFromBoW drives the reference's solver (src/LoopClosing.cc:685-696):
// SetRansacParameters(0.99, nBoWInliers, 300), then iterate(20, ...) until it converges or has no more iterations.  The stand-in
// KeyFrame lacks GetRotation, GetTranslation and isBad: the KeyFrame of this program derives from it and adds them.
// usage: dropin_sim3 <in.bin> <out.bin>
//   in : int32 fix_scale, form (0: the constructor of :35, 1: the one of :122), overload (0: iterate with bConverge, 1: without),
//        min_inliers, max_its, chunk, rig (1: KeyFrame 2 has a second camera), seed;
//        two KeyFrames: float R[9], t[3], cam[4], mvLevelSigma2[8];
//        int32 mN1, then per entry int32 flags, oct1, oct2, float Xw1[3], Xw2[3]
//        flags: 1 KeyFrame 1 holds a map point there, 2 a match exists, 4 / 8 the first / second point isBad, 16 / 32 the first / second
//        point is observed in its KeyFrame, 64 (form 1) the loop KeyFrame of the entry is null
//   out: int32 supported, n_chunks; per chunk int32 bNoMore, bConverge, nInliers, float T[16] (row major);
//        uint8 vbInliers[mN1] of the last chunk; float T12[16], R[9], t[3], s of the getters;
//        float Xc1[3 mN1], Xc2[3 mN1]: Rcw * Xw + tcw of every entry, in the stand-ins' arithmetic
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "sim3_stub_types.h"

#include "Sim3Solver_device.h"

namespace {
struct KF : ORB_SLAM3::KeyFrame {
    bool bad = false;
    Eigen::Matrix3f GetRotation() { return GetPose().rotationMatrix(); }
    Eigen::Vector3f GetTranslation() { return GetPose().translation(); }
    bool isBad() { return bad; }
};
typedef std::shared_ptr<KF> KFp;
typedef std::shared_ptr<ORB_SLAM3::MapPoint> MPp;
typedef ORB_SLAM3::msorb_host::Sim3Solver<KFp, MPp, Eigen::Matrix4f, sim3_stub::Matrix3f, sim3_stub::Vector3f> Solver;
template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t hdr[8];
    if (!rd(in, hdr, 8)) return 3;
    const bool fix_scale = hdr[0] != 0;
    const int form = hdr[1], overload = hdr[2], min_inliers = hdr[3], max_its = hdr[4], chunk = hdr[5], rig = hdr[6];
    DUtils::Random::SeedRand(hdr[7]);
    KFp kf[2];
    ORB_SLAM3::GeometricCamera cams[2], second;
    for (int k = 0; k < 2; k++) {
        float R[9], t[3], c[4], s2[8];
        if (!rd(in, R, 9) || !rd(in, t, 3) || !rd(in, c, 4) || !rd(in, s2, 8)) return 3;
        kf[k] = std::make_shared<KF>();
        kf[k]->mnId = 10 + k;
        Eigen::Matrix3f Rm;
        std::memcpy(Rm.m, R, sizeof(R));
        kf[k]->SetPose(Sophus::SE3f(Rm, Eigen::Vector3f{{t[0], t[1], t[2]}}));
        cams[k].fx = c[0]; cams[k].fy = c[1]; cams[k].cx = c[2]; cams[k].cy = c[3];
        kf[k]->mpCamera = &cams[k];
        kf[k]->mvLevelSigma2.assign(s2, s2 + 8);
    }
    if (rig) kf[1]->mpCamera2 = &second;
    int32_t mN1 = 0;
    if (!rd(in, &mN1, 1) || mN1 < 0) return 3;
    std::vector<int32_t> flags(mN1), oct1(mN1), oct2(mN1);
    std::vector<float> Xw1(3 * (size_t)mN1), Xw2(3 * (size_t)mN1);
    for (int i = 0; i < mN1; i++)
        if (!rd(in, &flags[i], 1) || !rd(in, &oct1[i], 1) || !rd(in, &oct2[i], 1) || !rd(in, &Xw1[3 * (size_t)i], 3) || !rd(in, &Xw2[3 * (size_t)i], 3))
            return 3;
    fclose(in);
    std::vector<cv::KeyPoint> kps1(mN1), kps2(mN1);
    std::vector<unsigned char> desc((size_t)mN1 * 32);
    for (int i = 0; i < mN1; i++) { kps1[i].octave = oct1[i]; kps2[i].octave = oct2[i]; }
    kf[0]->SetFeatures(kps1, desc.data());
    kf[1]->SetFeatures(kps2, desc.data());
    std::vector<MPp> matched12(mN1), points1(mN1);
    std::vector<KFp> kfs1(mN1, kf[0]), kfs2(mN1, kf[1]);
    for (int i = 0; i < mN1; i++) {
        const float* a = &Xw1[3 * (size_t)i];
        const float* b = &Xw2[3 * (size_t)i];
        if (flags[i] & 1) {
            auto p = std::make_shared<ORB_SLAM3::MapPoint>();
            p->pos = Eigen::Vector3f{{a[0], a[1], a[2]}};
            p->mbBad = (flags[i] & 4) != 0;
            if (flags[i] & 16) p->obsIdx[kf[0].get()] = i;
            kf[0]->AddMapPoint(p, i);
            points1[i] = p;
        }
        if (flags[i] & 2) {
            auto p = std::make_shared<ORB_SLAM3::MapPoint>();
            p->pos = Eigen::Vector3f{{b[0], b[1], b[2]}};
            p->mbBad = (flags[i] & 8) != 0;
            if (flags[i] & 32) p->obsIdx[kf[1].get()] = i;
            matched12[i] = p;
        }
        if (flags[i] & 64) kfs2[i] = nullptr;
    }
    std::unique_ptr<Solver> solver;
    if (form == 0) solver.reset(new Solver(kf[0], kf[1], matched12, fix_scale));
    else solver.reset(new Solver(kf[0], kf[1], kfs1, points1, kfs2, matched12, fix_scale));
    std::vector<int32_t> head;
    std::vector<float> mats;
    std::vector<bool> vbInliers;
    int n_chunks = 0;
    if (solver->supported()) {
        solver->SetRansacParameters(0.99, min_inliers, max_its);   // LoopClosing.cc:686
        bool bNoMore = false, bConverge = false;
        int nInliers = 0;
        while (!bConverge && !bNoMore && n_chunks < 1000) {        // :693-696
            const Eigen::Matrix4f T = overload == 0 ? solver->iterate(chunk, bNoMore, vbInliers, nInliers, bConverge)
                                                    : solver->iterate(chunk, bNoMore, vbInliers, nInliers);
            if (overload == 1) bConverge = nInliers > 0;   // the first overload says so only through nInliers
            head.push_back(bNoMore); head.push_back(bConverge); head.push_back(nInliers);
            mats.insert(mats.end(), T.m, T.m + 16);
            n_chunks++;
        }
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    const int32_t h2[2] = {solver->supported() ? 1 : 0, n_chunks};
    fwrite(h2, 4, 2, out);
    for (int k = 0; k < n_chunks; k++) { fwrite(&head[3 * (size_t)k], 4, 3, out); fwrite(&mats[16 * (size_t)k], 4, 16, out); }
    std::vector<uint8_t> vb(mN1, 0);
    for (size_t i = 0; i < vbInliers.size() && i < (size_t)mN1; i++) vb[i] = vbInliers[i];
    fwrite(vb.data(), 1, vb.size(), out);
    const Eigen::Matrix4f T12 = solver->GetEstimatedTransformation();
    const Eigen::Matrix3f R = solver->GetEstimatedRotation();
    const Eigen::Vector3f t = solver->GetEstimatedTranslation();
    const float s = solver->GetEstimatedScale();
    fwrite(T12.m, 4, 16, out); fwrite(R.m, 4, 9, out); fwrite(t.v, 4, 3, out); fwrite(&s, 4, 1, out);
    for (int k = 0; k < 2; k++) {
        const std::vector<float>& Xw = k ? Xw2 : Xw1;
        const Eigen::Matrix3f Rcw = kf[k]->GetRotation();
        const Eigen::Vector3f tcw = kf[k]->GetTranslation();
        for (int i = 0; i < mN1; i++) {
            const Eigen::Vector3f X = Rcw * Eigen::Vector3f{{Xw[3 * (size_t)i], Xw[3 * (size_t)i + 1], Xw[3 * (size_t)i + 2]}} + tcw;
            fwrite(X.v, 4, 3, out);
        }
    }
    return fclose(out) == 0 ? 0 : 3;
}
