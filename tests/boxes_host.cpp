// boxes_host.cpp -- the rule of frr_query_boxes (f_renderer_amd/csrc/frr_boxes.h, whose rule part compiles with no HIP) in a
// program of its own, for tests/test_boxes_cpu.py to build under the host sanitizers:
//   boxes_host <W> <H> <mvps.f32> <lo_hi.f32> <flags.u32> <depth.f32>
// mvps: nitems x 16, lo_hi: nitems x 6, flags: nitems, depth: W x H.  Over the windows and the world-2 ownership masks of
// tests/box_scenes.py (WINDOWS, then ROW_MASKS in sorted key order), with out_entries = nitems + 3 allocated exactly, it
// prints the values of one case per line, then "boxes_host: ok <cases>".  It also checks what needs no second opinion: the
// entries behind the items are zero, the status array agrees with the values, and a run with out_entries = 0 writes nothing.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <vector>

#include "../f_renderer_amd/csrc/frr_boxes.h"

template <typename T> static std::vector<T> read_all(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::cerr << "cannot open " << path << "\n"; std::exit(2); }
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(raw.size() / sizeof(T));
    for (size_t k = 0; k < v.size(); ++k) v[k] = *reinterpret_cast<const T *>(raw.data() + sizeof(T) * k);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 7) { std::cerr << "usage: boxes_host W H mvps.f32 lo_hi.f32 flags.u32 depth.f32\n"; return 2; }
    const int32_t W = (int32_t)std::strtol(argv[1], nullptr, 10), H = (int32_t)std::strtol(argv[2], nullptr, 10);
    const std::vector<float> mvps = read_all<float>(argv[3]), lo_hi = read_all<float>(argv[4]), depth = read_all<float>(argv[6]);
    const std::vector<uint32_t> flags = read_all<uint32_t>(argv[5]);
    const uint64_t n = flags.size();
    if (W != 128 || H != 96 || mvps.size() != 16 * n || lo_hi.size() != 6 * n || depth.size() != (size_t)W * (size_t)H) { std::cerr << "bad input\n"; return 2; }
    const int32_t win[][4] = {{0, W, 0, H}, {3, 125, 5, 91}, {17, 82, 33, 70}, {40, 41, 50, 51}, {0, W, 47, 48}, {64, 65, 0, H}, {1, 36, 2, 35}};
    const uint8_t masks[][3] = {{1, 0, 1}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}};   // (0, False), (0, True), (1, False), (1, True)
    int cases = 0;
    const size_t nwin = sizeof win / sizeof win[0], nmask = sizeof masks / sizeof masks[0];
    for (size_t k = 0; k < nwin + nmask; ++k) {
        const int32_t *w = win[k < nwin ? k : 0];
        const uint8_t *own = k < nwin ? nullptr : masks[k - nwin];
        const frr::BoxWindow bw = {(uint32_t)W, (uint32_t)H, w[0], w[1], w[2], w[3]};
        std::vector<uint32_t> out(n + 3, 0xDEADBEEFu);   // (exactly out_entries: a write past the end is the sanitizer's to find)
        std::vector<int32_t> srl(6 * n, -1);
        if (frr::box_host_query(mvps.data(), lo_hi.data(), flags.data(), n, bw, depth.data(), own, out.data(), out.size(), srl.data()) != (int64_t)n) return 1;
        for (uint64_t i = 0; i < n + 3; ++i) {
            if (i >= n) { if (out[i] != 0u) { std::printf("boxes_host: entry %llu behind the items is not zero\n", (unsigned long long)i); return 1; } continue; }
            const int32_t st = srl[6 * i];
            const bool zero = st == frr::BOX_NONE || st == frr::BOX_OUTSIDE || st == frr::BOX_HIDDEN;
            if (st < 0 || st > frr::BOX_UNBOUNDED || zero != (out[i] == 0u)) { std::printf("boxes_host: item %llu: status %d with value %u\n", (unsigned long long)i, st, out[i]); return 1; }
        }
        std::vector<uint32_t> none;
        frr::box_host_query(mvps.data(), lo_hi.data(), flags.data(), n, bw, depth.data(), own, none.data(), 0, nullptr);
        for (uint64_t i = 0; i < n + 3; ++i) std::printf("%u%c", out[i], i + 1 == n + 3 ? '\n' : ' ');
        ++cases;
    }
    std::printf("boxes_host: ok %d\n", cases);
    return 0;
}
