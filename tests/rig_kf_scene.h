// The scene reader of the two-camera KeyFrame mains (tests/dropin_rig_kf_main.cc, tests/dropin_rig_kf_search_main.cc): camera
// models, scale tables and KeyFrames of a two-camera rig (KeyFrame::SetRig of tests/slam_stub) from the binary the Python tests write.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"

namespace rig_kf_scene {
using namespace ORB_SLAM3;
typedef std::shared_ptr<MapPoint> MP;

template <class T>
inline std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(3); }
    return v;
}
template <class T>
inline void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }
inline void wri(FILE* f, int v) { fwrite(&v, 4, 1, f); }

inline Sophus::SE3f se3(const std::vector<float>& p, int at) {
    Eigen::Matrix3f R; Eigen::Vector3f t;
    memcpy(R.m, &p[at], 36); memcpy(t.v, &p[at + 9], 12);
    return Sophus::SE3f(R, t);
}

struct Scene {
    std::vector<float> scale, sigma2, inv_sigma2;
    GeometricCamera cam[2];
    float bounds[4], mbf;
};

inline std::shared_ptr<KeyFrame> read_kf(FILE* f, int NL, int NR, Scene& S, unsigned long id, std::vector<MP>& held_out) {
    const int N = NL + NR;
    const auto kl = rd<cv::KeyPoint>(f, NL), kr = rd<cv::KeyPoint>(f, NR);
    const auto desc = rd<unsigned char>(f, (size_t)N * 32);
    const auto node = rd<int>(f, N);
    const auto held = rd<unsigned char>(f, N);
    const auto held_obs = rd<int>(f, N);
    const auto pose = rd<float>(f, 24);   // Tcw: R(9) t(3); Trl: R(9) t(3)
    auto kf = std::make_shared<KeyFrame>();
    kf->SetRig(kl, kr, desc.data(), se3(pose, 12));
    kf->SetPose(se3(pose, 0));
    kf->mnId = id;
    kf->mvScaleFactors = S.scale; kf->mvLevelSigma2 = S.sigma2; kf->mvInvLevelSigma2 = S.inv_sigma2;
    kf->mnScaleLevels = (int)S.scale.size(); kf->mfLogScaleFactor = std::log(1.2f); kf->mbf = S.mbf;
    kf->mpCamera = &S.cam[0]; kf->mpCamera2 = &S.cam[1];
    kf->mnMinX = (int)S.bounds[0]; kf->mnMaxX = (int)S.bounds[1]; kf->mnMinY = (int)S.bounds[2]; kf->mnMaxY = (int)S.bounds[3];
    DBoW2::FeatureVector fv;
    for (int i = 0; i < N; i++) if (node[i] >= 0) fv.addFeature((DBoW2::NodeId)node[i], (unsigned)i);
    kf->SetFeatureVector(fv);
    for (int i = 0; i < N; i++)
        if (held[i]) {
            auto p = std::make_shared<MapPoint>();
            p->mnId = id * 100000ul + (unsigned long)i;
            p->nObs = held_obs[i];
            p->obsIdx[kf.get()] = i;
            kf->AddMapPoint(p, i);
            held_out.push_back(p);
        }
    return kf;
}

}  // namespace rig_kf_scene
