// ms-slam_amd/csrc/sim3_select.h (the sequential rule of Sim3Solver::iterate, src/Sim3Solver.cc:344-366 of the reference) and
// ms-slam_amd/csrc/sim3_device.h (ComputeSim3 / CheckInliers) on the host.
//
//   sim3_select_main select in.bin
//     in : int32 n_cases, then per case int32 n, min_inliers, best_in, counts[n]
//     Every case goes through sim3_select, through sim3_select_continue in pieces of 1, 7 and 64, and through a literal restatement
//     of the loop with the reference's members; any difference prints the case and exits with 1.  Prints one line per case:
//     winner converged consumed best.
//   sim3_select_main eval in.bin out.bin
//     in : int32 n, H, fix_scale; float cam1[4], cam2[4], X1[3 n], X2[3 n], max_err1[n], max_err2[n]; int32 triples[3 H]
//     out: int32 counts[H]; float (s, R[9], t[3])[H]; uint8 mask[H][n]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sim3_device.h"
#include "sim3_select.h"

namespace {

// :319-372 with the members it touches, hypotheses already evaluated
msorb::Sim3Selection literal(const std::vector<int>& mnInliers, int mRansacMinInliers, int mnBestInliers) {
    int mnIterations = 0, winner = -1;
    const int mRansacMaxIts = (int)mnInliers.size();
    bool bConverge = false;
    while (mnIterations < mRansacMaxIts) {
        const int mnInliersi = mnInliers[mnIterations];
        mnIterations++;
        if (mnInliersi >= mnBestInliers) {
            mnBestInliers = mnInliersi;
            winner = mnIterations - 1;
            if (mnInliersi > mRansacMinInliers) {
                bConverge = true;
                break;
            }
        }
    }
    return msorb::Sim3Selection{winner, bConverge ? 1 : 0, mnIterations, mnBestInliers};
}

bool equal(const msorb::Sim3Selection& a, const msorb::Sim3Selection& b) {
    return a.winner == b.winner && a.converged == b.converged && a.consumed == b.consumed && a.best == b.best;
}

template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int run_select(FILE* in) {
    int32_t n_cases = 0;
    if (!rd(in, &n_cases, 1)) return 2;
    for (int k = 0; k < n_cases; k++) {
        int32_t hdr[3];
        if (!rd(in, hdr, 3) || hdr[0] < 0) return 2;
        std::vector<int> counts(hdr[0]);
        if (!rd(in, counts.data(), counts.size())) return 2;
        const int n = hdr[0];
        const msorb::Sim3Selection a = msorb::sim3_select(counts.data(), n, hdr[1], hdr[2]), want = literal(counts, hdr[1], hdr[2]);
        bool ok = equal(a, want);
        for (int piece : {1, 7, 64}) {
            msorb::Sim3Selection s{-1, 0, n, hdr[2]};
            for (int base = 0; base < n; base += piece) {
                std::vector<int> chunk(counts.begin() + base, counts.begin() + std::min(n, base + piece));   // its own block: a read past it is caught
                msorb::sim3_select_continue(s, chunk.data(), (int)chunk.size(), base, hdr[1]);
            }
            ok = ok && equal(s, want);
        }
        if (!ok) {
            std::printf("case %d (n %d min_inliers %d best_in %d) differs from the literal loop\n", k, n, hdr[1], hdr[2]);
            return 1;
        }
        std::printf("%d %d %d %d\n", a.winner, a.converged, a.consumed, a.best);
    }
    return 0;
}

int run_eval(FILE* in, const char* out_path) {
    int32_t hdr[3];
    float cam1[4], cam2[4];
    if (!rd(in, hdr, 3) || !rd(in, cam1, 4) || !rd(in, cam2, 4) || hdr[0] < 3 || hdr[1] < 1) return 2;
    const int n = hdr[0], H = hdr[1];
    std::vector<float> X1(3 * (size_t)n), X2(3 * (size_t)n), e1(n), e2(n);
    std::vector<int32_t> tr(3 * (size_t)H);
    if (!rd(in, X1.data(), X1.size()) || !rd(in, X2.data(), X2.size()) || !rd(in, e1.data(), n) || !rd(in, e2.data(), n) ||
        !rd(in, tr.data(), tr.size()))
        return 2;
    std::vector<int32_t> counts(H);
    std::vector<float> rec(13 * (size_t)H);
    std::vector<uint8_t> mask((size_t)H * n);
    for (int h = 0; h < H; h++) {
        float P1[9], P2[9];
        for (int i = 0; i < 3; i++) {
            const int idx = tr[3 * (size_t)h + i];
            if (idx < 0 || idx >= n) return 2;
            std::memcpy(P1 + 3 * i, &X1[3 * (size_t)idx], 12);
            std::memcpy(P2 + 3 * i, &X2[3 * (size_t)idx], 12);
        }
        msorb::Sim3Transform T;
        msorb::sim3_compute(P1, P2, hdr[2] != 0, T);
        int c = 0;
        for (int i = 0; i < n; i++) {
            const bool in_ = msorb::sim3_is_inlier(T, cam1, cam2, &X1[3 * (size_t)i], &X2[3 * (size_t)i], e1[i], e2[i]);
            mask[(size_t)h * n + i] = in_;
            c += in_;
        }
        counts[h] = c;
        float* r = &rec[13 * (size_t)h];
        r[0] = T.s;
        std::memcpy(r + 1, T.R, 36);
        std::memcpy(r + 10, T.t, 12);
    }
    FILE* out = std::fopen(out_path, "wb");
    if (!out) return 2;
    std::fwrite(counts.data(), 4, counts.size(), out);
    std::fwrite(rec.data(), 4, rec.size(), out);
    std::fwrite(mask.data(), 1, mask.size(), out);
    return std::fclose(out) == 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[2], "rb");
    if (!in) return 2;
    int rc = 2;
    if (!std::strcmp(argv[1], "select")) rc = run_select(in);
    else if (!std::strcmp(argv[1], "eval") && argc == 4) rc = run_eval(in, argv[3]);
    std::fclose(in);
    return rc;
}
