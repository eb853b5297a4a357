// ms-slam_amd/csrc/two_view_device.h and two_view_select.h, the text the kernels compile, built for the host and run serially.
//   two_view_main run <scenes.bin> <out.bin>      every scene through tests/two_view_host_path.h (files of tests/two_view_cases.py)
//   two_view_main select <cases.bin> <out.bin>    the three rules of two_view_select.h on small inputs:
//       int32 count, per case int32 kind, then
//       kind 0 (fold):   int32 n, float scores[n]                                           -> float score, int32 winner
//       kind 1 (branch): float SH, SF, double h_ratio                                       -> int32 branch, float RH
//       kind 2 / 3 (final F / H): int32 n_inliers, min_triangulated, float min_parallax,
//                        int32 n_good[4 / 8], float parallax[4 / 8]                         -> int32 chosen, int32 0
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "two_view_host_path.h"

namespace {

std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> b;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
    uint8_t buf[65536];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
    std::fclose(f);
    return b;
}

struct Reader {
    const std::vector<uint8_t>& b;
    size_t o = 0;
    template <class T> std::vector<T> take(size_t n) {
        if (o + n * sizeof(T) > b.size()) { std::fprintf(stderr, "short input\n"); std::exit(2); }
        std::vector<T> v(n);
        if (n) std::memcpy(v.data(), b.data() + o, n * sizeof(T));
        o += n * sizeof(T);
        return v;
    }
};

struct Writer {
    std::vector<uint8_t> b;
    template <class T> void put(const T* p, size_t n) {
        const uint8_t* q = reinterpret_cast<const uint8_t*>(p);
        b.insert(b.end(), q, q + n * sizeof(T));
        while (b.size() % 4) b.push_back(0);
    }
};

int run(Reader& in, Writer& out) {
    const int scenes = in.take<int>(1)[0];
    for (int s = 0; s < scenes; s++) {
        const std::vector<int> hd = in.take<int>(4);
        const std::vector<float> fl = in.take<float>(6);
        tv_host::Problem p;
        p.n1 = hd[0]; p.n2 = hd[1]; p.n_hyp = hd[2]; p.min_triangulated = hd[3];
        std::memcpy(p.cam, fl.data(), 16);
        p.sigma = fl[4]; p.min_parallax = fl[5];
        p.h_ratio = in.take<double>(1)[0];
        p.keys1 = in.take<float>(2 * (size_t)p.n1);
        p.keys2 = in.take<float>(2 * (size_t)p.n2);
        p.matches12 = in.take<int>(p.n1);
        p.sets = in.take<int>(8 * (size_t)p.n_hyp);
        const tv_host::Answer a = tv_host::reconstruct(p);
        const tv_host::Answer b = tv_host::reconstruct(p, 2);   // the reference's two threads: the same bits
        if (std::memcmp(&a.r, &b.r, sizeof a.r) || a.scores != b.scores || a.masks != b.masks || a.p3d != b.p3d) {
            std::fprintf(stderr, "scene %d: two threads differ from one\n", s);
            return 1;
        }
        out.put(&a.r, 1);
        out.put(a.triangulated.data(), a.triangulated.size());
        out.put(a.p3d.data(), a.p3d.size());
        out.put(a.inliers.data(), a.inliers.size());
        out.put(a.scores.data(), a.scores.size());
        out.put(a.counts.data(), a.counts.size());
        out.put(a.masks.data(), a.masks.size());
        out.put(a.status.data(), a.status.size());
    }
    return 0;
}

int select(Reader& in, Writer& out) {
    const int cases = in.take<int>(1)[0];
    for (int c = 0; c < cases; c++) {
        const int kind = in.take<int>(1)[0];
        if (kind == 0) {
            const int n = in.take<int>(1)[0];
            const std::vector<float> s = in.take<float>(n);
            msorb::TvFold whole{0.0f, -1}, parts{0.0f, -1};
            msorb::tv_fold_continue(whole, s.data(), n, 0);
            for (int base = 0; base < n; base += 7) msorb::tv_fold_continue(parts, s.data() + base, n - base < 7 ? n - base : 7, base);   // as the kernel folds its chunks
            if (std::memcmp(&whole, &parts, sizeof whole)) { std::fprintf(stderr, "case %d: the fold in pieces differs from the whole\n", c); return 1; }
            out.put(&whole.score, 1);
            out.put(&whole.winner, 1);
        } else if (kind == 1) {
            const std::vector<float> s = in.take<float>(2);
            const double h_ratio = in.take<double>(1)[0];
            float RH;
            const int b = msorb::tv_branch(s[0], s[1], h_ratio, RH);
            out.put(&b, 1);
            out.put(&RH, 1);
        } else {
            const int k = kind == 2 ? 4 : 8;
            const std::vector<int> hd = in.take<int>(2);
            const float min_parallax = in.take<float>(1)[0];
            const std::vector<int> good = in.take<int>(k);
            const std::vector<float> par = in.take<float>(k);
            const int r[2] = {kind == 2 ? msorb::tv_final_f(good.data(), par.data(), hd[0], min_parallax, hd[1])
                                        : msorb::tv_final_h(good.data(), par.data(), hd[0], min_parallax, hd[1]), 0};
            out.put(r, 2);
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: two_view_main run|select <in> <out>\n"); return 2; }
    const std::vector<uint8_t> b = slurp(argv[2]);
    Reader in{b};
    Writer out;
    const std::string mode = argv[1];
    const int rc = mode == "run" ? run(in, out) : mode == "select" ? select(in, out) : 2;
    if (rc) return rc;
    FILE* f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.b.data(), 1, out.b.size(), f) != out.b.size()) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    std::fclose(f);
    return 0;
}
