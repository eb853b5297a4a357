// ms-slam_amd/csrc/mlpnp_device.h and mlpnp_select.h, the text the kernels compile, built for the host and run serially (lane 0 of 1).
//   mlpnp_main run <problems.bin> <out.bin>     every hypothesis of every scene, then the rule (files of tests/mlpnp_cases.py)
//   mlpnp_main select <cases.bin> <out.bin>     int32 count, per case: n, min_inliers, best_in, counts[n] -> 5 int32 per case
//   mlpnp_main jac <cases.bin> <out.bin>        int32 count, per case 12 doubles w, T, p, n -> 7 doubles: residual, Jacobian row
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../ms-slam_amd/csrc/mlpnp_device.h"
#include "../ms-slam_amd/csrc/mlpnp_select.h"

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
    template <class T> void put(const T* p, size_t n) { const uint8_t* q = reinterpret_cast<const uint8_t*>(p); b.insert(b.end(), q, q + n * sizeof(T)); }
    void align8() { while (b.size() % 8) b.push_back(0); }
};

struct Result { int winner, converged, consumed, n_inliers; float Tcw[16]; double R[9], t[3]; };
static_assert(sizeof(Result) == 176, "msorb_mlpnp_result");

int run(Reader& in, Writer& out) {
    const int scenes = in.take<int>(1)[0];
    for (int s = 0; s < scenes; s++) {
        const std::vector<int> hd = in.take<int>(4);
        const int n = hd[0], H = hd[1];
        const std::vector<float> cam = in.take<float>(4), p2d = in.take<float>(2 * (size_t)n), p3d = in.take<float>(3 * (size_t)n), err = in.take<float>(n);
        const std::vector<int> sets = in.take<int>(6 * (size_t)H);
        std::vector<int> counts(H);
        std::vector<uint8_t> flags(H), masks((size_t)H * n);
        std::vector<double> poses(12 * (size_t)H);
        msorb::MlpnpWork work;
        for (int h = 0; h < H; h++) {
            double* R = &poses[12 * (size_t)h];
            flags[h] = (uint8_t)msorb::mlpnp_compute_pose(work, 0, 1, cam.data(), p2d.data(), p3d.data(), &sets[6 * (size_t)h], R, R + 9);
            int c = 0;
            for (int i = 0; i < n; i++) {
                const bool in_ = msorb::mlpnp_is_inlier(R, R + 9, cam.data(), &p3d[3 * (size_t)i], &p2d[2 * (size_t)i], err[i]);
                masks[(size_t)h * n + i] = in_;
                c += in_;
            }
            counts[h] = c;
        }
        const msorb::MlpnpSelection sel = msorb::mlpnp_select(counts.data(), H, hd[2], hd[3]);
        Result r{};
        r.winner = sel.winner; r.converged = sel.converged; r.consumed = sel.consumed;
        std::vector<uint8_t> inl(n, 0);
        if (sel.winner >= 0) {
            const double* P = &poses[12 * (size_t)sel.winner];
            r.n_inliers = counts[sel.winner];
            for (int k = 0; k < 9; k++) r.R[k] = P[k];
            for (int k = 0; k < 3; k++) r.t[k] = P[9 + k];
            for (int row = 0; row < 3; row++) {
                for (int c = 0; c < 3; c++) r.Tcw[4 * row + c] = (float)P[3 * row + c];
                r.Tcw[4 * row + 3] = (float)P[9 + row];
            }
            r.Tcw[15] = 1.0f;
            std::memcpy(inl.data(), &masks[(size_t)sel.winner * n], n);
        }
        out.put(&r, 1);
        out.put(counts.data(), H);
        out.put(flags.data(), H);
        out.align8();
        out.put(poses.data(), poses.size());
        out.put(inl.data(), n);
        out.align8();
    }
    return 0;
}

int select(Reader& in, Writer& out) {
    const int cases = in.take<int>(1)[0];
    for (int c = 0; c < cases; c++) {
        const std::vector<int> hd = in.take<int>(3);
        const std::vector<int> counts = in.take<int>(hd[0]);
        const msorb::MlpnpSelection whole = msorb::mlpnp_select(counts.data(), hd[0], hd[1], hd[2]);
        // and in pieces of 7, as the selection kernel folds its chunks
        msorb::MlpnpSelection sel{-1, 0, hd[0], hd[2], -1};
        for (int base = 0; base < hd[0]; base += 7) msorb::mlpnp_select_continue(sel, counts.data() + base, hd[0] - base < 7 ? hd[0] - base : 7, base, hd[1]);
        if (std::memcmp(&whole, &sel, sizeof sel)) { std::fprintf(stderr, "case %d: the fold differs from the whole\n", c); return 1; }
        const int r[5] = {whole.winner, whole.converged, whole.consumed, whole.best, whole.best_h};
        out.put(r, 5);
    }
    return 0;
}

int jac(Reader& in, Writer& out) {
    const int cases = in.take<int>(1)[0];
    for (int c = 0; c < cases; c++) {
        const std::vector<double> v = in.take<double>(12);
        double R[9], o[7];
        msorb::mlpnp_rodrigues2rot(v.data(), R);
        o[0] = msorb::mlpnp_residual_and_jacobian(R, v.data(), v.data() + 3, v.data() + 6, v.data() + 9, o + 1);
        const double r = msorb::mlpnp_residual(R, v.data() + 3, v.data() + 6, v.data() + 9);
        if (std::memcmp(&r, &o[0], 8)) { std::fprintf(stderr, "case %d: the two residuals differ\n", c); return 1; }
        out.put(o, 7);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: mlpnp_main run|select|jac <in> <out>\n"); return 2; }
    const std::vector<uint8_t> b = slurp(argv[2]);
    Reader in{b};
    Writer out;
    const std::string mode = argv[1];
    const int rc = mode == "run" ? run(in, out) : mode == "select" ? select(in, out) : mode == "jac" ? jac(in, out) : 2;
    if (rc) return rc;
    FILE* f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.b.data(), 1, out.b.size(), f) != out.b.size()) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    std::fclose(f);
    return 0;
}
