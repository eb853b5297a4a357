// The KeyFrame searches of the drop-in ORB_SLAM3::ORBmatcher CLASS on KeyFrames of a two-camera rig (KeyFrame::NLeft != -1, mpCamera2
// set), compiled against the stand-ins of tests/slam_stub:
//   ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches), F a two-camera frame                        ORBmatcher.cc:223-421 (GetKeyPoint, :335, :359)
//   ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12)                                               ORBmatcher.cc:872-1016 (rule :907-909, :929-931)
//   ORBmatcher::SearchByBoW(pKF1, pKF2, ..., nCurrentId), the loop form                            ORBmatcher.cc:1018-1166 (rule :1054-1056, :1078-1080)
//   ORBmatcher::SearchByProjection(F, pKF, sAlreadyFound, th, ORBdist), relocalisation               ORBmatcher.cc:2154-2275
// The frame is KeyFrame 2's features as a two-camera frame (left keypoints / rows first, then the right camera's).
// usage: dropin_rig_kf_search <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "ORBmatcher.h"
#include "ORBmatcher_device.h"
#include "rig_kf_scene.h"

using namespace ORB_SLAM3;
using namespace rig_kf_scene;

// map point -> index of the feature that held it when the scene was read (read_kf: mnId = KeyFrame id * 100000 + index), -1 for none
static int feature_of(const MP& p, unsigned long kf_id) {
    return p && p->mnId / 100000ul == kf_id ? (int)(p->mnId % 100000ul) : -1;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    const auto hdr = rd<int>(f, 6);   // NL1 NR1 NL2 NR2 - nlevels
    const int NL1 = hdr[0], NR1 = hdr[1], NL2 = hdr[2], NR2 = hdr[3], nl = hdr[5], N1 = NL1 + NR1, N2 = NL2 + NR2;
    const auto fl = rd<float>(f, 16);  // cam0 fx fy cx cy | cam1 fx fy cx cy | minX maxX minY maxY | th ORBdist nnratio nCurrentId
    Scene S;
    S.scale = rd<float>(f, nl); S.sigma2 = rd<float>(f, nl);
    S.inv_sigma2.resize(nl);
    for (int l = 0; l < nl; l++) S.inv_sigma2[l] = 1.0f / S.sigma2[l];
    for (int c = 0; c < 2; c++) { S.cam[c].fx = fl[4 * c]; S.cam[c].fy = fl[4 * c + 1]; S.cam[c].cx = fl[4 * c + 2]; S.cam[c].cy = fl[4 * c + 3]; S.cam[c].id = c + 1; }
    memcpy(S.bounds, &fl[8], 16);
    S.mbf = 0.0f;
    const float th = fl[12], nnratio = fl[14];
    const int orb_dist = (int)fl[13];
    unsigned long nCurrentId = (unsigned long)fl[15];
    std::vector<MP> held1, held2;
    auto kf1 = read_kf(f, NL1, NR1, S, 1, held1);
    auto kf2 = read_kf(f, NL2, NR2, S, 2, held2);
    const auto loop1 = rd<unsigned char>(f, N1), loop2 = rd<unsigned char>(f, N2);   // map points already used for this loop candidate
    const auto pos1 = rd<float>(f, (size_t)3 * N1), maxd1 = rd<float>(f, N1), mind1 = rd<float>(f, N1);
    const auto mdesc1 = rd<unsigned char>(f, (size_t)N1 * 32);
    const auto found1 = rd<unsigned char>(f, N1);                                   // sAlreadyFound
    const auto fpose = rd<float>(f, 12);                                            // the frame's Tcw: R(9) t(3)
    fclose(f);
    for (auto& p : held1) {
        const int i = feature_of(p, 1);
        memcpy(p->pos.v, &pos1[(size_t)3 * i], 12);
        p->mfMaxDistance = maxd1[i]; p->mfMinDistance = mind1[i];
        memcpy(p->descriptor, &mdesc1[(size_t)32 * i], 32);
    }

    // KeyFrame 2's features as a two-camera frame (tests/dropin_rig_main.cc set_rig)
    Frame F;
    {
        std::vector<cv::KeyPoint> kl(NL2), kr(NR2);
        for (int i = 0; i < NL2; i++) kl[i] = kf2->GetKey(i);
        for (int i = 0; i < NR2; i++) kr[i] = kf2->GetKeyRight(i);
        std::vector<cv::KeyPoint> all = kl;
        all.insert(all.end(), kr.begin(), kr.end());
        std::vector<unsigned char> desc((size_t)N2 * 32);
        for (int i = 0; i < N2; i++) memcpy(&desc[(size_t)32 * i], kf2->GetDescriptor(i).ptr<unsigned char>(0), 32);
        F.SetFeatures(all, desc.data());
        F.mvKeys = kl; F.mvKeysUn = kl; F.mvKeysRight = kr;
        F.Nleft = NL2; F.Nright = NR2;
        F.mFeatVec = kf2->GetFeatureVector();
        F.mvScaleFactors = S.scale; F.mvLevelSigma2 = S.sigma2; F.mvInvLevelSigma2 = S.inv_sigma2;
        F.mnScaleLevels = nl; F.mfLogScaleFactor = std::log(1.2f);
        F.mpCamera = &S.cam[0]; F.mpCamera2 = &S.cam[1];
        F.mnMinX = S.bounds[0]; F.mnMaxX = S.bounds[1]; F.mnMinY = S.bounds[2]; F.mnMaxY = S.bounds[3];
        F.mvbOutlier.assign(N2, false);
        F.mTcw = se3(fpose, 0);
        F.mnId = 300;
    }
    FILE* o = fopen(argv[2], "wb");
    for (int ori = 1; ori >= 0; ori--) {
        ORBmatcher matcher(nnratio, ori != 0);
        // ---- SearchByBoW(pKF, F): vpMapPointMatches as KeyFrame 1 feature indices
        std::vector<MP> vpMatches;
        const int nb = matcher.SearchByBoW(kf1, F, vpMatches);
        std::vector<int> ids(vpMatches.size());
        for (size_t j = 0; j < vpMatches.size(); j++) ids[j] = feature_of(vpMatches[j], 1);
        wri(o, nb); wri(o, (int)ids.size()); wr(o, ids);
        // ---- SearchByBoW(pKF1, pKF2, vpMatches12): KeyFrame 2 feature indices
        std::vector<MP> vpMatches12;
        const int nk = matcher.SearchByBoW(kf1, kf2, vpMatches12);
        std::vector<int> m12(vpMatches12.size());
        for (size_t i = 0; i < vpMatches12.size(); i++) m12[i] = feature_of(vpMatches12[i], 2);
        wri(o, nk); wri(o, (int)m12.size()); wr(o, m12);
    }
    // ---- the loop form, with the map points marked as already used for this candidate
    {
        for (auto& p : held1) p->mnLoopPointForKF = loop1[feature_of(p, 1)] ? nCurrentId : 0;
        for (auto& p : held2) p->mnLoopPointForKF = loop2[feature_of(p, 2)] ? nCurrentId : 0;
        ORBmatcher matcher(nnratio, true);
        std::vector<std::shared_ptr<KeyFrame>> cKF, lKF;
        std::vector<MP> cMP, lMP;
        const int nw = matcher.SearchByBoW(kf1, kf2, cKF, cMP, lKF, lMP, nCurrentId);
        std::vector<int> c(cMP.size()), l(lMP.size());
        int consistent = cKF.size() == cMP.size() && lKF.size() == lMP.size() && cMP.size() == lMP.size();
        for (size_t k = 0; k < cMP.size(); k++) {
            c[k] = feature_of(cMP[k], 1);
            consistent &= cKF[k] == kf1 && cMP[k]->mnLoopPointForKF == nCurrentId;
        }
        for (size_t k = 0; k < lMP.size(); k++) {
            l[k] = feature_of(lMP[k], 2);
            consistent &= lKF[k] == kf2 && lMP[k]->mnLoopPointForKF == nCurrentId;
        }
        wri(o, nw); wri(o, (int)c.size()); wr(o, c); wr(o, l); wri(o, consistent);
    }
    // ---- SearchByProjection(F, pKF1, sAlreadyFound, th, ORBdist): the projection table the class computes first, then the search
    for (int ori = 1; ori >= 0; ori--) {
        std::set<MP> found;
        for (auto& p : held1) if (found1[feature_of(p, 1)]) found.insert(p);
        msorb_host::KeyFrameProjection P;
        msorb_host::ProjectKeyFramePoints(F, kf1, found, P);
        F.mvpMapPoints.assign(N2, MP());
        ORBmatcher matcher(nnratio, ori != 0);
        const int np = matcher.SearchByProjection(F, kf1, found, th, orb_dist);
        std::vector<int> ids(N2);
        for (int j = 0; j < N2; j++) ids[j] = feature_of(F.mvpMapPoints[j], 1);
        wri(o, np); wr(o, ids);
        wr(o, P.valid); wr(o, P.u); wr(o, P.v); wr(o, P.level); wr(o, P.angle);
    }
    fclose(o);
    msorb_host::Shutdown();
    return 0;
}
