// ORB_SLAM3::msorb_host::CreateNewMapPoints (ms-slam_amd/host/LocalMapping_device.h) compiled against the stand-ins of tests/slam_stub and run
// on a scene of tests/new_map_points_cases.py.  The stand-in KeyFrame lacks GetDepth, invfx / invfy and ComputeSceneMedianDepth:
// the KeyFrame of this program derives from it and adds them.
// usage: dropin_newpoints <in.bin> <out.bin> <stop_before> <rig>
//   stop_before: checkNewKeyFrames() answers true when asked before neighbour `stop_before` (-1: never)
//   rig: 1 = neighbour 1 gets a second camera
//   in : int32 K, bCoarse, bInertial, bFarPoints; float thFarPoints; then K + 1 KeyFrames (the current one first), each:
//        int32 n; cv::KeyPoint[n]; uint8 desc[n][32]; float u_right[n], depth[n]; int32 node[n] (-1: in no list);
//        uint8 has_point[n]; float R[9], t[3], fx, fy, cx, cy, mb, mbf; behind them, per KeyFrame, float mvScaleFactors[8],
//        mvLevelSigma2[8]
//   out: int32 returned, n_log; per neighbour float F12[9], ep[2], Ow[3] (K + 1 times Ow, the current KeyFrame first, F12 / ep zero
//        for it); then n_log records of int32 (neighbour, idx1, idx2) + uint32 x3D bits [3]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "slam_stub_types.h"

#include "LocalMapping_device.h"

namespace {
struct KF : ORB_SLAM3::KeyFrame {
    float invfx = 0, invfy = 0;
    float GetDepth(size_t idx) { return mvDepth[idx]; }
    void SetDepth(const std::vector<float>& d) { mvDepth = d; }
    float ComputeSceneMedianDepth(int) { return 10.0f; }
};
template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    const int stop_before = atoi(argv[3]), rig = atoi(argv[4]);
    int32_t hdr[4];
    float th_far = 0;
    if (!rd(in, hdr, 4) || !rd(in, &th_far, 1)) return 3;
    const int K = hdr[0];
    std::vector<std::shared_ptr<KF>> kfs;
    std::vector<ORB_SLAM3::GeometricCamera> cams(K + 1);
    ORB_SLAM3::GeometricCamera second;
    for (int k = 0; k <= K; k++) {
        int32_t n = 0;
        if (!rd(in, &n, 1) || n < 0) return 3;
        std::vector<cv::KeyPoint> kps(n);
        std::vector<unsigned char> desc((size_t)n * 32), has(n);
        std::vector<float> ur(n), depth(n);
        std::vector<int32_t> node(n);
        float R[9], t[3], c[6];
        static_assert(sizeof(cv::KeyPoint) == 28, "cv::KeyPoint layout");
        if (!rd(in, kps.data(), n) || !rd(in, desc.data(), desc.size()) || !rd(in, ur.data(), n) || !rd(in, depth.data(), n) ||
            !rd(in, node.data(), n) || !rd(in, has.data(), n) || !rd(in, R, 9) || !rd(in, t, 3) || !rd(in, c, 6)) return 3;
        auto kf = std::make_shared<KF>();
        kf->mnId = 100 + k;
        kf->SetFeatures(kps, desc.data());
        kf->SetuRight(ur);
        kf->SetDepth(depth);
        DBoW2::FeatureVector fv;
        for (int i = 0; i < n; i++)
            if (node[i] >= 0) fv.addFeature((DBoW2::NodeId)node[i], (unsigned)i);
        kf->SetFeatureVector(fv);
        for (int i = 0; i < n; i++)
            if (has[i]) kf->AddMapPoint(std::make_shared<ORB_SLAM3::MapPoint>(), i);
        Eigen::Matrix3f Rm;
        std::memcpy(Rm.m, R, sizeof(R));
        kf->SetPose(Sophus::SE3f(Rm, Eigen::Vector3f{{t[0], t[1], t[2]}}));
        kf->fx = c[0]; kf->fy = c[1]; kf->cx = c[2]; kf->cy = c[3]; kf->mb = c[4]; kf->mbf = c[5];
        kf->invfx = 1.0f / kf->fx; kf->invfy = 1.0f / kf->fy;
        cams[k].fx = c[0]; cams[k].fy = c[1]; cams[k].cx = c[2]; cams[k].cy = c[3];
        kf->mpCamera = &cams[k];
        kf->mvScaleFactors.assign(8, 1.0f);
        kf->mvLevelSigma2.assign(8, 1.0f);
        kfs.push_back(kf);
    }
    // mvScaleFactors / mvLevelSigma2 exactly as the Python side has them
    for (int k = 0; k <= K; k++)
        if (!rd(in, kfs[k]->mvScaleFactors.data(), 8) || !rd(in, kfs[k]->mvLevelSigma2.data(), 8)) return 3;
    fclose(in);
    if (rig && K >= 2) kfs[2]->mpCamera2 = &second;
    std::vector<std::shared_ptr<KF>> neigh(kfs.begin() + 1, kfs.end());
    std::vector<int32_t> log;
    int asked = 0;   // the neighbour the next question is asked before
    int ret = 0;
    {
        ORB_SLAM3::msorb_host::KeyFrameStore store(0);
        ret = ORB_SLAM3::msorb_host::CreateNewMapPoints(
            store, kfs[0], neigh, /*bMonocular*/ false, hdr[2] != 0, hdr[1] != 0, hdr[3] != 0, th_far,
            [&] { return ++asked == stop_before; },
            [&](const float* x3D, const std::shared_ptr<KF>& pKF2, int idx1, int idx2) {   // LocalMapping.cc:715-730 in miniature
                auto pMP = std::make_shared<ORB_SLAM3::MapPoint>();
                pMP->pos = Eigen::Vector3f{{x3D[0], x3D[1], x3D[2]}};
                pMP->AddObservation(kfs[0], idx1);
                pMP->AddObservation(pKF2, idx2);
                kfs[0]->AddMapPoint(pMP, idx1);
                pKF2->AddMapPoint(pMP, idx2);
                int32_t rec[6] = {(int32_t)(pKF2->mnId - 101), idx1, idx2, 0, 0, 0};
                std::memcpy(rec + 3, x3D, 12);
                log.insert(log.end(), rec, rec + 6);
            });
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    const int32_t head[2] = {ret, (int32_t)(log.size() / 6)};
    fwrite(head, 4, 2, out);
    for (int k = 0; k <= K; k++) {
        float g[14] = {0};
        if (k > 0 && !rig) ORB_SLAM3::msorb_host::TriangulationGeometry(kfs[0], kfs[k], g, g + 9);
        const auto Ow = kfs[k]->GetCameraCenter();
        g[11] = Ow(0); g[12] = Ow(1); g[13] = Ow(2);
        fwrite(g, 4, 14, out);
    }
    fwrite(log.data(), 4, log.size(), out);
    return fclose(out) == 0 ? 0 : 3;
}
