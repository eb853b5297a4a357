// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:414-733) on the device: the loop over the neighbours — search, parallax
// test, triangulation or stereo unprojection, the depth, reprojection and scale gates — as ONE msorb_create_new_map_points_kf call
// on resident KeyFrames.  What stays in LocalMapping.cc is the choice of the neighbours (:417-434) and the body that makes a
// MapPoint out of a position (:715-730), handed in as onNewPoint.  INTEGRATION.md section 3 has the edit.
//
// Not covered: KeyFrames with a second camera (:526-576 pick one of four pose pairs per match and triangulate through
// KannalaBrandt8) — the function then returns false without touching anything and the caller runs the reference's loop.
#pragma once
#include <cstdint>
#include <vector>

#include "ORBmatcher_device.h"

namespace ORB_SLAM3 {
namespace msorb_host {

namespace detail {
// a KeyFrame's geometry block and its per-feature stereo measurements (GetuRight / GetDepth: mvuRight / mvDepth are protected)
template <class KeyFramePtr>
void NewPointsGeometry(const KeyFramePtr& pKF, msorb_new_points_geometry& g, std::vector<float>& u_right, std::vector<float>& depth) {
    const auto Tcw = pKF->GetPose();
    const auto R = Tcw.rotationMatrix();
    const auto t = Tcw.translation();
    const auto Ow = pKF->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) g.Tcw[4 * r + c] = R(r, c);
        g.Tcw[4 * r + 3] = t(r);
        g.Ow[r] = Ow(r);
    }
    g.fx = pKF->fx; g.fy = pKF->fy; g.cx = pKF->cx; g.cy = pKF->cy;
    g.invfx = pKF->invfx; g.invfy = pKF->invfy;
    g.mb = pKF->mb; g.mbf = pKF->mbf;
    const int n = pKF->GetN();
    u_right.resize(n);
    depth.resize(n);
    for (int i = 0; i < n; i++) { u_right[i] = pKF->GetuRight(i); depth[i] = pKF->GetDepth(i); }
    g.u_right = u_right.data();
    g.depth = depth.data();
}
template <class KeyFramePtr>
std::vector<uint8_t> WithoutMapPoint(const KeyFramePtr& pKF) {   // ORBmatcher.cc:1237-1241 / :1264-1266 with bOnlyStereo = false
    const auto mps = pKF->GetMapPointMatches();
    std::vector<uint8_t> free_(mps.size());
    for (size_t i = 0; i < mps.size(); i++) free_[i] = !mps[i];
    return free_;
}
}  // namespace detail

// The loop of :460-731 over vpNeighKFs.  checkNewKeyFrames() is polled before every neighbour but the first, as :462-463 does:
// when it fires the function returns, and the points of the remaining neighbours (computed already) are not created.
// onNewPoint(const float x3D[3], pKF2, idx1, idx2) is called for every new point in the reference's order — the neighbours in
// turn, inside one the matches by ascending idx1 (the order of vMatchedIndices, ORBmatcher.cc:1385-1393) — and runs :715-730.
// Returns false, with nothing done, when any KeyFrame involved has mpCamera2 (or a neighbour is listed twice or is the current
// KeyFrame): the caller then runs the reference's loop.
template <class KeyFramePtr, class CheckNewKeyFrames, class OnNewPoint>
bool CreateNewMapPoints(KeyFrameStore& store, const KeyFramePtr& pKFcur, const std::vector<KeyFramePtr>& vpNeighKFs, bool bMonocular,
                        bool bInertial, bool bCoarse, bool bFarPoints, float thFarPoints, CheckNewKeyFrames checkNewKeyFrames,
                        OnNewPoint onNewPoint) {
    if (pKFcur->mpCamera2) return false;
    for (const KeyFramePtr& pKF2 : vpNeighKFs)
        if (pKF2->mpCamera2) return false;
    const size_t K = vpNeighKFs.size();
    const auto Ow1 = pKFcur->GetCameraCenter();
    std::vector<int> slot(K, -1);   // the neighbour's place in the call; -1: dropped by the baseline test
    std::vector<KeyFramePtr> kept;
    for (size_t i = 0; i < K; i++) {
        const KeyFramePtr& pKF2 = vpNeighKFs[i];
        const auto Ow2 = pKF2->GetCameraCenter();   // :469-486
        const auto vBaseline = Ow2 - Ow1;
        const float baseline = vBaseline.norm();
        if (!bMonocular) {
            if (baseline < pKF2->mb) continue;
        } else {
            const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
            const float ratioBaselineDepth = baseline / medianDepthKF2;
            if (ratioBaselineDepth < 0.01) continue;
        }
        bool twice = &*pKF2 == &*pKFcur;   // (GetBestCovisibilityKeyFrames and the walk of :423-434 list a KeyFrame once, never the
        for (const KeyFramePtr& q : kept) twice = twice || &*q == &*pKF2;   // current one; the entry refuses anything else)
        if (twice) return false;
        slot[i] = (int)kept.size();
        kept.push_back(pKF2);
    }
    const size_t M = kept.size();
    const KeyFrameStore::Lease l1 = store.Ensure(pKFcur);
    std::vector<KeyFrameStore::Lease> l2(M);   // held until the call has returned
    const std::vector<uint8_t> valid1 = detail::WithoutMapPoint(pKFcur);
    std::vector<std::vector<uint8_t>> avail2(M);
    std::vector<std::vector<float>> ur(M + 1), depth(M + 1);
    msorb_new_points_call call{};
    call.kf1 = l1->id;
    call.valid1 = valid1.data();
    detail::NewPointsGeometry(pKFcur, call.g1, ur[M], depth[M]);
    call.coarse = bCoarse;
    call.check_orientation = false;   // ORBmatcher matcher(th, false) (:438)
    call.inertial = bInertial;
    call.th_far = bFarPoints ? thFarPoints : 0.0f;
    const size_t n1 = valid1.size();
    std::vector<msorb_new_points_neighbour> nb(M);
    std::vector<int> match12(M * n1);
    std::vector<uint8_t> status(M * n1);
    std::vector<float> x3D(M * n1 * 3);
    for (size_t k = 0; k < M; k++) {
        msorb_new_points_neighbour& N = nb[k];
        N = msorb_new_points_neighbour{};
        l2[k] = store.Ensure(kept[k]);
        N.kf2 = l2[k]->id;
        avail2[k] = detail::WithoutMapPoint(kept[k]);
        N.avail2 = avail2[k].data();
        detail::NewPointsGeometry(kept[k], N.g2, ur[k], depth[k]);
        TriangulationGeometry(pKFcur, kept[k], N.F12, N.ep);
        N.match12 = match12.data() + k * n1;
        N.status = status.data() + k * n1;
        N.x3D = x3D.data() + k * n1 * 3;
    }
    check(msorb_create_new_map_points_kf(store.get(), &call, nb.data(), (int)M, nullptr), "msorb_create_new_map_points_kf");
    for (size_t i = 0; i < K; i++) {
        if (i > 0 && checkNewKeyFrames()) return true;   // :462-463
        if (slot[i] < 0) continue;
        const msorb_new_points_neighbour& N = nb[slot[i]];
        for (size_t idx1 = 0; idx1 < n1; idx1++)
            if (N.status[idx1] >= MSORB_NP_TRIANGULATED && N.status[idx1] <= MSORB_NP_STEREO2)
                onNewPoint(N.x3D + 3 * idx1, vpNeighKFs[i], (int)idx1, N.match12[idx1]);
    }
    return true;
}

}  // namespace msorb_host
}  // namespace ORB_SLAM3
