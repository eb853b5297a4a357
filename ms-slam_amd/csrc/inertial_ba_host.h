// What the C entries of the three inertial bundle adjustments (local_inertial_ba.hip, inertial_ba_engine.hip) do on the host in the
// same way: carving a block, the finite checks of their common records, and the outputs of a call that moved nothing.  Host code
// only: no kernel reads this.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "local_inertial_ba_device.h"

namespace msorb {
namespace iba_host {

struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += up16(bytes); return o; }
};

inline bool finite_all(const double* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}
inline bool finite_all(const float* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// false, with the last error set to prefix + what was met: KeyFrames, then inertial edges, then points and observations
inline bool inputs_finite(const char* prefix, int K, const msorb_iba_keyframe* kfs, int NI, const msorb_iba_inertial_edge* iedges, int P,
                          const float* pos_w, int E, const float* xy, const float* u_right, const float* inv_sigma2) {
    const char* what = nullptr;
    for (int k = 0; k < K && !what; k++)
        if (!finite_all(kfs[k].Rwb, 48) || !finite_all(&kfs[k].fx, (size_t)5)) what = "a non-finite value in a KeyFrame";
    for (int i = 0; i < NI && !what; i++)
        if (!finite_all(iedges[i].pre.dR, (size_t)67) || !finite_all(iedges[i].pre.info, 81) || !finite_all(iedges[i].info_gyro, 18))
            what = "a non-finite value in an inertial edge";
    if (!what && (!finite_all(pos_w, 3 * (size_t)P) || !finite_all(xy, 2 * (size_t)E) || !finite_all(u_right, (size_t)E) ||
                  !finite_all(inv_sigma2, (size_t)E)))
        what = "a non-finite value in a point or an observation";
    if (what) set_last_error(std::string(prefix) + what);
    return !what;
}

// a call that moved nothing: every output repeats its input and no flag is set (edge_outlier, point_included: where the routine
// has them)
inline void repeat_inputs(int K, const msorb_iba_keyframe* kfs, int P, const float* pos_w, int E, msorb_iba_keyframe_out* kf_out,
                          float* pos_out, double* pos_d, uint8_t* edge_outlier, uint8_t* point_included) {
    for (int k = 0; k < K; k++) {
        pinert::Vertices V;
        liba::vertices_from(V, kfs[k]);
        liba::keyframe_out(V, kf_out[k]);
    }
    for (size_t i = 0; i < 3 * (size_t)P; i++) {
        pos_out[i] = pos_w[i];
        if (pos_d) pos_d[i] = (double)pos_w[i];
    }
    if (point_included && P) std::memset(point_included, 0, (size_t)P);
    if (edge_outlier && E) std::memset(edge_outlier, 0, (size_t)E);
}

}  // namespace iba_host
}  // namespace msorb
