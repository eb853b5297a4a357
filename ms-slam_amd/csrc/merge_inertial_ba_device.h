// Optimizer::MergeInertialBA (src/Optimizer.cc:3918-4420) after its gathering loops, for pinhole KeyFrames without a second camera:
// the welding bundle adjustment of two inertial maps.  The graph is FullInertialBA's init = 0 form (full_inertial_ba_device.h) with
// one more kind of KeyFrame, and the passes are that header's; this one states what MergeInertialBA does differently.  The same
// text is read by hipcc (merge_inertial_ba.hip) and by g++ (tests/merge_inertial_ba_main.cc), with -ffp-contract=off.  DESIGN.md
// section 26.
//
//   vertices   kind 0: both temporal windows and the covisible KeyFrame an inertial edge reaches, 15 unknowns; kind 3: every other
//              covisible KeyFrame: its VertexPose is free, its velocity and bias vertices are in the graph but no edge reaches
//              them, so g2o's active set leaves them out (sparse_optimizer.cpp, initializeOptimization): 6 unknowns; kind 1 / 2:
//              fixed.  Unknowns: [6 per free KeyFrame | 9 per free KeyFrame of kind 0], both ascending.
//   edges      EdgeInertial with Huber sqrt(16.92) and its information as given, EdgeGyroRW, EdgeAccRW (:4141-4185); EdgeMono /
//              EdgeStereo with the information mvInvLevelSigma2[octave] (:4272, :4293).
//   loop       setUserLambdaInit(1e3) (:4047), optimize(8) (:4317), the stop flag installed before it (:4309-4314).
//   flags      chi2() > 5.991f (mono), > 7.815f (stereo) and nothing else (:4322-4349): no depth test.  chi2() is read without
//              computeError(): it belongs to the copy the last trial wrote, accepted or not (local_inertial_ba_device.h, classify).
#pragma once
#include "full_inertial_ba_device.h"

namespace msorb {
namespace miba {

using fiba::Problem;
using fiba::Res;
using fiba::Work;
using pinert::Vertices;

constexpr double kLambdaInit = 1e3;
constexpr int kIterations = 8;
inline int capacity() { return fiba::kMaxN; }   // unknowns

inline void plan_problem(int K, const msorb_iba_keyframe* kfs, int NI, const msorb_iba_inertial_edge* ie, int n_points, int n_edges,
                         const int* edge_kf, const int* edge_point, Problem& q) {
    fiba::plan_problem(0, K, kfs, NI, ie, n_points, n_edges, edge_kf, edge_point, q, 3);
}

// :4331, :4345: the float thresholds against the double chi2 the last trial left
SE3_HD uint8_t classify(const liba::Work& W, int e) { return W.chi2[e] > (W.ur[e] >= 0 ? (double)7.815f : (double)5.991f) ? 1 : 0; }

template <typename Exec>
SE3_HD void pass_classify(Exec& ex, const Work& F, uint8_t* outlier) {
    for (int e = ex.tid(); e < F.L.E; e += ex.stride()) outlier[e] = classify(F.L, e);
}

// what a KeyFrame's output holds: a free one that is a vertex (row >= 0) its estimate, of kind 3 the pose alone (its velocity and
// biases come back as they went in, :4398-4406); every other one its input
inline void keyframe_result(const msorb_iba_keyframe& in, int row, const Vertices& est, msorb_iba_keyframe_out& o) {
    Vertices V;
    liba::vertices_from(V, in);
    if (row >= 0 && in.kind == 0) V = est;
    else if (row >= 0) V.P = est.P;
    liba::keyframe_out(V, o);
}

}  // namespace miba
}  // namespace msorb
