// What the host layer of the drop-in matcher hands the device for KeyFrames and frames of a two-camera rig (KeyFrame::NLeft != -1,
// Frame::Nleft != -1), compared with the reference's own reading of the same features, on the CPU: only the flattening code of
// ms-slam_amd/host (BowSide, KeyFrameKeyPoints / FrameKeyPoints, ProjectKeyFramePoints) is instantiated, no msorb_* entry point, so
// the program never loads the HIP runtime.  Built with -D_GLIBCXX_ASSERTIONS (and optionally -fsanitize=address): an index past the end
// of a keypoint vector aborts.
//   BowSide::FillKeyFrame      angle[i] = pKF->GetKeyPoint(i).angle for i < GetN()                ORBmatcher.cc:335, :359
//   BowSide::FillFrame         angle[i] = mvKeys[i] (i < Nleft), mvKeysRight[i - Nleft] beyond     ORBmatcher.cc:344-346, :365-367
//   BowSide::FillKeyFramePair  flag[i] = 0 for i >= NLeft on a two-camera KeyFrame                 ORBmatcher.cc:907-909, :929-931, :1054-1056, :1078-1080
//   ProjectKeyFramePoints      angle[i] = pKF->GetKeyPoint(i).angle (the in-bounds reading of :2238)
// Prints one line per failed check to stderr; exit status 0 = every check held.
// usage: rig_keyframe_host
#include <cstdio>
#include <memory>
#include <set>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "ORBmatcher_device.h"
#include "ORBmatcher_rig_device.h"

using namespace ORB_SLAM3;
typedef std::shared_ptr<MapPoint> MP;

static int g_fail = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                 \
            fprintf(stderr, "\n");                                        \
            g_fail++;                                                     \
        }                                                                 \
    } while (0)

static std::vector<cv::KeyPoint> keys(int n, float angle0, float x0) {
    std::vector<cv::KeyPoint> k(n);
    for (int i = 0; i < n; i++) {
        k[i].pt.x = x0 + 17.0f * i;
        k[i].pt.y = 40.0f + 5.0f * (i % 7);
        k[i].angle = angle0 + (float)i;
        k[i].octave = i % 3;
        k[i].size = 31;
    }
    return k;
}
static std::vector<unsigned char> descriptors(int n, int salt) {
    std::vector<unsigned char> d((size_t)n * 32);
    for (size_t b = 0; b < d.size(); b++) d[b] = (unsigned char)(b * 31 + salt);
    return d;
}
static DBoW2::FeatureVector every_feature(int n) {   // node i % 5 for feature i: every feature is in the FeatureVector
    DBoW2::FeatureVector fv;
    for (int i = 0; i < n; i++) fv.addFeature((DBoW2::NodeId)(i % 5), (unsigned)i);
    return fv;
}

int main() {
    const int NL = 6, NR = 9, N = NL + NR;   // more right-camera features than left ones: GetAllKeyUn() is the shorter vector
    GeometricCamera cam;
    cam.fx = 500; cam.fy = 500; cam.cx = 320; cam.cy = 240;
    const std::vector<float> scale = {1.0f, 1.2f, 1.44f, 1.728f, 2.0736f, 2.48832f, 2.985984f, 3.5831808f};

    // ---- a two-camera KeyFrame (KeyFrame.h:345-355): left angles 10.., right angles 200..
    auto kf = std::make_shared<KeyFrame>();
    const auto kl = keys(NL, 10.0f, 30.0f), kr = keys(NR, 200.0f, 35.0f);
    const auto kdesc = descriptors(N, 3);
    kf->SetRig(kl, kr, kdesc.data(), Sophus::SE3f());
    kf->SetFeatureVector(every_feature(N));
    kf->mpCamera = &cam; kf->mpCamera2 = &cam;
    kf->mvScaleFactors = scale; kf->mnScaleLevels = 8; kf->mfLogScaleFactor = std::log(1.2f);
    std::vector<MP> held;
    for (int i = 0; i < N; i++) {   // a good map point on every feature of both cameras
        auto p = std::make_shared<MapPoint>();
        p->mnId = 1000 + i;
        const cv::KeyPoint k = kf->GetKeyPoint(i);
        const float z = 10.0f;   // in front of the frame's camera (identity pose), projects back onto the keypoint
        p->pos = Eigen::Vector3f{{(k.pt.x - cam.cx) / cam.fx * z, (k.pt.y - cam.cy) / cam.fy * z, z}};
        p->mfMaxDistance = 20.0f; p->mfMinDistance = 5.0f;
        for (int b = 0; b < 32; b++) p->descriptor[b] = (unsigned char)(i + b);
        kf->AddMapPoint(p, i);
        held.push_back(p);
    }
    CHECK(kf->GetAllKeyUn().size() == (size_t)NL, "GetAllKeyUn() holds %zu keypoints", kf->GetAllKeyUn().size());

    // ---- BowSide::FillKeyFrame: GetKeyPoint(realIdxKF).angle for every feature
    {
        msorb_host::BowSide s;
        s.FillKeyFrame(kf);
        CHECK(s.angle.size() == (size_t)N, "%zu angles for N = %d", s.angle.size(), N);
        for (int i = 0; i < N && i < (int)s.angle.size(); i++)
            CHECK(s.angle[i] == kf->GetKeyPoint(i).angle, "KeyFrame feature %d: angle %g, GetKeyPoint %g", i, s.angle[i], kf->GetKeyPoint(i).angle);
        CHECK(s.desc.size() == (size_t)N * 32, "%zu descriptor bytes", s.desc.size());
        for (int i = 0; i < N && (size_t)i * 32 < s.desc.size(); i++)
            CHECK(std::memcmp(&s.desc[(size_t)i * 32], &kdesc[(size_t)i * 32], 32) == 0, "KeyFrame descriptor %d", i);
        const auto kp = msorb_host::KeyFrameKeyPoints(kf);   // what KeyFrameStore::Ensure uploads with n = GetN()
        CHECK(kp.size() == (size_t)N, "KeyFrameKeyPoints: %zu keypoints for N = %d", kp.size(), N);
        for (int i = 0; i < N && i < (int)kp.size(); i++)
            CHECK(kp[i].pt.x == kf->GetKeyPoint(i).pt.x && kp[i].angle == kf->GetKeyPoint(i).angle, "KeyFrameKeyPoints %d", i);
    }

    // ---- a two-camera Frame (Frame.h:226, 324-332), set up as tests/dropin_rig_main.cc does
    Frame F;
    const int FL = 5, FR = 8, FN = FL + FR;
    {
        const auto fl = keys(FL, 50.0f, 32.0f), fr = keys(FR, 300.0f, 36.0f);
        std::vector<cv::KeyPoint> all = fl;
        all.insert(all.end(), fr.begin(), fr.end());
        const auto fd = descriptors(FN, 11);
        F.SetFeatures(all, fd.data());
        F.mvKeys = fl; F.mvKeysUn = fl; F.mvKeysRight = fr;
        F.Nleft = FL; F.Nright = FR;
        F.mFeatVec = every_feature(FN);
        F.mvScaleFactors = scale; F.mnScaleLevels = 8; F.mfLogScaleFactor = std::log(1.2f);
        F.mpCamera = &cam; F.mpCamera2 = &cam;
        F.mnMinX = 0; F.mnMaxX = 640; F.mnMinY = 0; F.mnMaxY = 480;
        F.mvbOutlier.assign(FN, false);
    }
    {
        msorb_host::BowSide s;
        s.FillFrame(F);
        CHECK(s.angle.size() == (size_t)FN, "%zu frame angles for N = %d", s.angle.size(), FN);
        for (int i = 0; i < FN && i < (int)s.angle.size(); i++) {
            const float want = i < F.Nleft ? F.mvKeys[i].angle : F.mvKeysRight[i - F.Nleft].angle;
            CHECK(s.angle[i] == want, "frame feature %d: angle %g, want %g", i, s.angle[i], want);
        }
    }

    // ---- KeyFrame-to-KeyFrame sides: right-camera features never take part on a two-camera KeyFrame
    {
        const auto mps = kf->GetMapPointMatches();
        msorb_host::BowSide s;
        s.FillKeyFramePair(kf, mps);
        CHECK(s.flag.size() == (size_t)N, "%zu flags", s.flag.size());
        for (int i = 0; i < N && i < (int)s.flag.size(); i++)
            CHECK(s.flag[i] == (i < NL ? 1 : 0), "KeyFrame pair flag %d = %d", i, s.flag[i]);
    }
    // ---- the same on a one-camera KeyFrame: every feature with a good map point stays a candidate
    {
        auto mono = std::make_shared<KeyFrame>();
        const auto k = keys(N, 20.0f, 31.0f);
        mono->SetFeatures(k, kdesc.data());
        mono->SetFeatureVector(every_feature(N));
        for (int i = 0; i < N; i++)
            if (i % 3) mono->AddMapPoint(held[i], i);
        held[4]->mbBad = true;
        const auto mps = mono->GetMapPointMatches();
        msorb_host::BowSide s;
        s.FillKeyFramePair(mono, mps);
        for (int i = 0; i < N && i < (int)s.flag.size(); i++)
            CHECK(s.flag[i] == (i % 3 != 0 && i != 4 ? 1 : 0), "one-camera pair flag %d = %d", i, s.flag[i]);
        for (int i = 0; i < N && i < (int)s.angle.size(); i++) CHECK(s.angle[i] == k[i].angle, "one-camera angle %d", i);
        held[4]->mbBad = false;
    }

    // ---- SearchByProjection(F, pKF, sAlreadyFound, th, ORBdist): the KeyFrame angle of every projected map point, right camera included
    {
        std::set<MP> already = {held[1]};
        msorb_host::KeyFrameProjection P;
        msorb_host::ProjectKeyFramePoints(F, kf, already, P);
        CHECK(P.angle.size() == (size_t)N, "%zu projection angles", P.angle.size());
        int right_valid = 0;
        for (int i = 0; i < N && i < (int)P.valid.size(); i++) {
            CHECK(P.valid[i] == (i != 1 ? 1 : 0), "projection valid %d = %d", i, P.valid[i]);
            if (!P.valid[i]) continue;
            right_valid += i >= NL;
            CHECK(P.angle[i] == kf->GetKeyPoint(i).angle, "projection angle %d: %g, GetKeyPoint %g", i, P.angle[i], kf->GetKeyPoint(i).angle);
        }
        CHECK(right_valid == NR, "%d right-camera map points projected", right_valid);
    }

    if (g_fail) fprintf(stderr, "%d checks failed\n", g_fail);
    else printf("ok\n");
    return g_fail ? 1 : 0;
}
