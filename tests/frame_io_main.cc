// ms-slam_amd/csrc/frame_io.h on the CPU (no HIP header): the offsets of a frame's output block against the formulas written out
// here, and the staging planes of a two-image call over every combination of `staged` bits and pointer positions.
// Sections: block, planes.  Also built with -fsanitize=address,undefined by tests/test_frame_io_cpu.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "frame_io.h"

using msorb::FrameBlock;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static int section_block() {
    const int caps[] = {1, 2, 3, 657 /* 500 + 19 * 8 + 5: odd */, 2152};
    for (int cap : caps) {
        {   // two images, no stereo fields
            const size_t kp_bytes = (size_t)cap * sizeof(msorb_keypoint), o_desc = 2 * kp_bytes, out_bytes = o_desc + (size_t)2 * cap * 32;
            const FrameBlock b(cap, false);
            CHECK(b.kp_bytes == kp_bytes && b.o_desc == o_desc && b.out_bytes == out_bytes);
            CHECK(b.o_kps(0) == 0 && b.o_kps(1) == kp_bytes && b.o_descs(0) == o_desc && b.o_descs(1) == o_desc + (size_t)cap * 32);
            CHECK(b.o_ur == 0 && b.o_dp == 0 && b.o_oob == 0 && b.o_cnt == 0);
            CHECK(b.o_kps(1) + kp_bytes <= b.o_descs(0) && b.o_descs(0) + (size_t)cap * 32 <= b.o_descs(1) && b.o_descs(1) + (size_t)cap * 32 <= b.out_bytes);
        }
        {   // a stereo frame: [kps 2*cap][desc 2*cap*32][u_right cap][depth cap][n_oob][n_left][n_right]
            const size_t kp_bytes = (size_t)cap * sizeof(msorb_keypoint);
            const size_t o_desc = 2 * kp_bytes, o_ur = o_desc + (size_t)2 * cap * 32, o_dp = o_ur + (size_t)cap * 4,
                         o_oob = o_dp + (size_t)cap * 4, o_cnt = o_oob + 4, out_bytes = o_oob + 16;
            const FrameBlock b(cap, true);
            CHECK(b.kp_bytes == kp_bytes && b.o_desc == o_desc && b.o_ur == o_ur && b.o_dp == o_dp && b.o_oob == o_oob && b.o_cnt == o_cnt &&
                  b.out_bytes == out_bytes);
            // the regions in order, none overlapping the next, all inside out_bytes
            const size_t begin[] = {b.o_kps(0), b.o_kps(1), b.o_descs(0), b.o_descs(1), b.o_ur, b.o_dp, b.o_oob, b.o_cnt};
            const size_t bytes[] = {kp_bytes, kp_bytes, (size_t)cap * 32, (size_t)cap * 32, (size_t)cap * 4, (size_t)cap * 4, 4, 8};
            for (int r = 0; r < 8; r++) CHECK(begin[r] + bytes[r] <= (r + 1 < 8 ? begin[r + 1] : b.out_bytes));
        }
    }
    // the copy-out tail on a filled block: counts checked first (library capacity, then the caller's), then every region
    const int cap = 657;
    for (int stereo = 0; stereo < 2; stereo++) {
        const FrameBlock b(cap, stereo != 0);
        std::vector<uint8_t> o(b.out_bytes);
        for (size_t i = 0; i < o.size(); i++) o[i] = (uint8_t)(i * 131 + 7);
        const int n[2] = {657, 300};
        std::vector<msorb_keypoint> ka(cap), kb(cap);
        std::vector<uint8_t> da((size_t)cap * 32), db((size_t)cap * 32);
        std::vector<float> ur(cap), dp(cap);
        int oob = -5;
        msorb_keypoint* const kps[2] = {ka.data(), kb.data()};
        uint8_t* const desc[2] = {da.data(), db.data()};
        const int neg[2] = {3, -1};
        CHECK(std::string(b.copy_out(o.data(), neg, cap, kps, desc, ur.data(), dp.data(), &oob)) == "keypoint capacity exceeded");
        CHECK(std::string(b.copy_out(o.data(), n, 656, kps, desc, ur.data(), dp.data(), &oob)) == "caller capacity too small");
        const int both[2] = {-1, 5000};   // the library's own capacity is reported first
        CHECK(std::string(b.copy_out(o.data(), both, cap, kps, desc, ur.data(), dp.data(), &oob)) == "keypoint capacity exceeded");
        CHECK(oob == -5);
        CHECK(b.copy_out(o.data(), n, cap, kps, desc, ur.data(), dp.data(), stereo ? &oob : nullptr) == nullptr);
        CHECK(!memcmp(ka.data(), o.data(), (size_t)n[0] * sizeof(msorb_keypoint)));
        CHECK(!memcmp(kb.data(), o.data() + b.kp_bytes, (size_t)n[1] * sizeof(msorb_keypoint)));
        CHECK(!memcmp(da.data(), o.data() + b.o_desc, (size_t)n[0] * 32) && !memcmp(db.data(), o.data() + b.o_desc + (size_t)cap * 32, (size_t)n[1] * 32));
        if (stereo) {
            CHECK(!memcmp(ur.data(), o.data() + b.o_ur, (size_t)n[0] * 4) && !memcmp(dp.data(), o.data() + b.o_dp, (size_t)n[0] * 4));
            CHECK(!memcmp(&oob, o.data() + b.o_oob, 4));
            CHECK(b.copy_out(o.data(), n, cap, kps, desc, ur.data(), dp.data(), nullptr) == nullptr);   // n_oob is optional
        } else {
            CHECK(oob == -5);
        }
    }
    return 0;
}

static int section_planes() {
    const size_t pitch = 328, rows = 5, plane = pitch * rows;
    std::vector<uint8_t> arena(6 * plane);                 // the staging block sits in the middle of one allocation
    const uint8_t* const block = arena.data() + 2 * plane;
    // where a pointer may lie: outside the block (before / after it), plane 0, plane 1, inside the block but not a plane start
    const struct { const uint8_t* p; int plane; bool ok; } where[] = {
        {arena.data(), -1, true},           {block + 2 * plane, -1, true}, {block, 0, true},          {block + plane, 1, true},
        {block + 1, -1, false},             {block + plane - 1, -1, false}, {block + plane + pitch, -1, false}, {block - 1, -1, false},
    };
    const int n_where = (int)(sizeof(where) / sizeof(where[0]));
    int refused = 0, accepted = 0;
    for (int staged = 0; staged < 4; staged++)
        for (int a = 0; a < n_where; a++)
            for (int b = 0; b < n_where; b++) {
                const uint8_t* const src[2] = {where[a].p, where[b].p};
                const size_t stride[2] = {pitch, pitch};
                const int w[2] = {a, b};
                int got[2] = {-7, -7};
                const char* err = msorb::pair_staging_planes(block, plane, pitch, src, stride, staged, got);
                // the rule, written out: only staged images are looked at; one that overlaps the block must start a plane
                int own_plane[2] = {-1, -1};
                bool bad = false;
                for (int i = 0; i < 2; i++) {
                    if (!(staged & (1 << i))) continue;
                    if (!where[w[i]].ok) bad = true;
                    own_plane[i] = where[w[i]].plane;
                }
                if (bad) {
                    CHECK(err && std::string(err).find("must be a plane msorb_stage_image returned") != std::string::npos);
                    refused++;
                    continue;
                }
                CHECK(err == nullptr);
                accepted++;
                for (int i = 0; i < 2; i++) {
                    const int other = own_plane[1 - i];
                    const int want = other == i ? 1 - i : i;
                    CHECK(got[i] == want && (got[i] == 0 || got[i] == 1));
                    // an un-staged image never goes into a plane a staged image of the call occupies
                    if (!(staged & (1 << i)) && (staged & (1 << (1 - i)))) CHECK(got[i] != own_plane[1 - i]);
                }
                if (staged == 0) CHECK(got[0] == 0 && got[1] == 1);
            }
    CHECK(refused > 0 && accepted > 0);
    // a staged image at another pitch is refused before its position is looked at
    {
        const uint8_t* const src[2] = {block + 1, arena.data()};
        const size_t stride[2] = {pitch + 4, pitch};
        int got[2];
        const char* err = msorb::pair_staging_planes(block, plane, pitch, src, stride, 1, got);
        CHECK(err && std::string(err) == "msorb_extract_pair: a staged image must have the staging pitch");
        CHECK(msorb::pair_staging_planes(block, plane, pitch, src, stride, 2, got) == nullptr && got[0] == 0 && got[1] == 1);
    }
    return 0;
}

int main(int argc, char** argv) {
    const std::string s = argc > 1 ? argv[1] : "";
    int rc = 2;
    if (s == "block") rc = section_block();
    else if (s == "planes") rc = section_planes();
    if (rc == 0) std::printf("ok %s\n", s.c_str());
    return rc;
}
