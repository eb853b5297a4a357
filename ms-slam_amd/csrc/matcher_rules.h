// Small host rules of the reference's matcher that several entries share, free of HIP: the rotation histogram with its
// ComputeThreeMaxima pruning, the GetFeaturesInArea walk of a frame's grid, the left-camera window of a map point.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "window_query.h"

namespace msorb {

// bin of the rotation histogram for a match between keypoints with these angles (ORBmatcher.cc:2043-2050 and the like), or -1
// when it falls outside [0, kHistoLength) (a NaN / out-of-range angle: the reference asserts)
inline int rotation_bin(float angle_a, float angle_b) {
    float rot = angle_a - angle_b;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)std::round(rot * (1.0f / kHistoLength));
    if (bin == kHistoLength) bin = 0;
    return bin >= 0 && bin < kHistoLength ? bin : -1;
}

// rotHist[HISTO_LENGTH] of the reference: entries per bin in insertion order; the matches that CheckOrientation withdraws are
// the entries outside the three fullest bins (ComputeThreeMaxima, ORBmatcher.cc:2129-2149 and the like)
struct RotationHistogram {
    std::vector<int> bins[kHistoLength];
    void push(int bin, int entry) {   // bin -1 (rotation_bin): the entry stays out of the histogram
        if (bin >= 0) bins[bin].push_back(entry);
    }
    template <typename Visit>
    void for_each_outside_three_maxima(Visit visit) const {
        int sizes[kHistoLength], ind[3];
        for (int i = 0; i < kHistoLength; i++) sizes[i] = (int)bins[i].size();
        msorb_three_maxima(sizes, kHistoLength, ind);
        for (int i = 0; i < kHistoLength; i++)
            if (i != ind[0] && i != ind[1] && i != ind[2])
                for (int e : bins[i]) visit(e);
    }
};

// A frame's grid on the host (cell = ix * kGridRows + iy, keypoint indices in ascending order inside a cell)
struct HostGrid {
    const msorb_keypoint* kps;
    const int *cell_begin, *cell_idx;
    float minX, minY, gridWInv, gridHInv;
};
// Frame::GetFeaturesInArea (Frame.cc:589-655): visit(idx) for every keypoint inside the box |dx| < r, |dy| < r on levels
// [min_level, max_level] (max_level < 0: no upper bound), in the reference's order; visit returns false to end the walk
template <typename Visit>
void walk_features_in_area(const HostGrid& g, float x, float y, float r, int min_level, int max_level, Visit visit) {
    const int minCX = std::max(0, (int)std::floor((x - g.minX - r) * g.gridWInv));
    if (minCX >= kGridCols) return;
    const int maxCX = std::min(kGridCols - 1, (int)std::ceil((x - g.minX + r) * g.gridWInv));
    if (maxCX < 0) return;
    const int minCY = std::max(0, (int)std::floor((y - g.minY - r) * g.gridHInv));
    if (minCY >= kGridRows) return;
    const int maxCY = std::min(kGridRows - 1, (int)std::ceil((y - g.minY + r) * g.gridHInv));
    if (maxCY < 0) return;
    const bool check = (min_level > 0) || (max_level >= 0);
    for (int ix = minCX; ix <= maxCX; ix++)
        for (int iy = minCY; iy <= maxCY; iy++) {
            const int c = ix * kGridRows + iy;
            for (int j = g.cell_begin[c]; j < g.cell_begin[c + 1]; j++) {
                const msorb_keypoint& kp = g.kps[g.cell_idx[j]];
                if (check) {
                    if (kp.octave < min_level) continue;
                    if (max_level >= 0 && kp.octave > max_level) continue;
                }
                if (std::fabs(kp.x - x) < r && std::fabs(kp.y - y) < r)
                    if (!visit(g.cell_idx[j])) return;
            }
        }
}

// the left-camera window of a map point in SearchByProjection(F, MapPoints) (ORBmatcher.cc:61-75): RadiusByViewingCos (:215-221)
// scaled by th and the predicted level's scale factor, levels [level - 1, level], the mbSparsified bypass of the occupancy test
inline WinQuery map_point_left_query(float x, float y, float ur, int level, float view_cos, float th, const float* scale, bool sparsified) {
    WinQuery w{};
    float r = (view_cos > 0.998) ? 2.5 : 4.0;
    if (th != 1.0) r *= th;
    w.x = x; w.y = y;
    w.r = r * scale[level];
    w.ur = ur;
    w.min_level = (int16_t)(level - 1);
    w.max_level = (int16_t)level;
    w.flags = kQValid | (sparsified ? 0 : kQSkipOccupied);
    return w;
}

}  // namespace msorb
