// Host twin of msorb_debug_decomp: ms-slam_amd/csrc/decomp_probe_device.h, the text decomp_probe.hip compiles, through g++ and
// glibc, one lane of one.
//   g++ -std=c++17 -O2 -ffp-contract=off tests/decomp_probe_main.cc -o decomp_probe_main
//   decomp_probe_main in.bin out.bin
// in.bin:  int32 n_blocks, then per block: int32 op, int32 n, n * in_width(op) doubles
// out.bin: per block n * 24 doubles.  Native endianness.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../ms-slam_amd/csrc/decomp_probe_device.h"

int main(int argc, char** argv) {
    using namespace msorb::decompprobe;
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* fi = std::fopen(argv[1], "rb");
    FILE* fo = fi ? std::fopen(argv[2], "wb") : nullptr;
    if (!fi || !fo) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t blocks = 0;
    if (std::fread(&blocks, 4, 1, fi) != 1 || blocks < 0) return 3;
    for (int b = 0; b < blocks; b++) {
        int32_t head[2];
        if (std::fread(head, 4, 2, fi) != 2 || head[0] < 0 || head[0] >= kDecompOps || head[1] < 0) return 3;
        const int op = head[0], n = head[1], w = in_width(op);
        std::vector<double> in((size_t)n * w), out((size_t)n * kDecompOut);
        if (n && std::fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 3;
        for (int i = 0; i < n; i++) record_one_lane(op, in.data() + (size_t)i * w, out.data() + (size_t)i * kDecompOut);
        if (n && std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 4;
    }
    std::fclose(fi);
    return std::fclose(fo) == 0 ? 0 : 4;
}
