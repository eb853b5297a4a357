// Plain definitions of the window search shared by the kernels (through matcher_device.h) and the HIP-free host rules
// (claim_replay.h, matcher_rules.h): constants of the reference, the query a window search takes and the list it returns.
#pragma once
#include <stdint.h>

#include "../../include/msorb.h"

namespace msorb {

constexpr int kGridCols = 64, kGridRows = 48;  // FRAME_GRID_COLS / FRAME_GRID_ROWS, Frame.h:44-45
constexpr int kThHigh = 100, kThLow = 50, kHistoLength = 30;  // ORBmatcher.cc:35-37
constexpr int kTopK = 8;  // candidates kept per query: with 4 a busy frame needed 4-5 device rounds (exhausted lists), with 8 fewer

constexpr uint8_t kQValid = 1, kQSkipOccupied = 2, kQFuseGate = 4, kQNoUr = 8;
struct WinQuery {
    float x, y, r, ur;
    int16_t min_level, max_level;
    uint8_t flags, pad[3];
};
struct TopK {
    int idx[kTopK];
    int dist[kTopK];
};

}  // namespace msorb
