// visible_host.cpp -- the span logic of frr_visible_pixels (f_renderer_amd/csrc/frr_visible.h, which compiles with no HIP)
// in a program of its own, for tests/test_visible_cpu.py to build under the host sanitizers:
//   visible_host <W> <H> <ids.u32> <bounds.u32>
// ids.u32: W x H triangle ids; bounds.u32: nitems + 1 item boundaries.  Over the full window and a set of sub-windows, per
// item and per triangle, with out_entries below, at and above the number of units, it compares visible_counts_host with
// the definition taken one entry at a time, prints "visible_host: ok <cases>" and exits 0 only if every count agrees.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <vector>

#include "../f_renderer_amd/csrc/frr_visible.h"

static std::vector<uint32_t> read_u32(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::cerr << "cannot open " << path << "\n"; std::exit(2); }
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<uint32_t> v(raw.size() / 4);
    for (size_t k = 0; k < v.size(); ++k) v[k] = *reinterpret_cast<const uint32_t *>(raw.data() + 4 * k);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 5) { std::cerr << "usage: visible_host W H ids.u32 bounds.u32\n"; return 2; }
    const int32_t W = (int32_t)std::strtol(argv[1], nullptr, 10), H = (int32_t)std::strtol(argv[2], nullptr, 10);
    const std::vector<uint32_t> ids = read_u32(argv[3]), bounds = read_u32(argv[4]);
    if (W < 1 || H < 1 || ids.size() != (size_t)W * (size_t)H || bounds.empty()) { std::cerr << "bad input\n"; return 2; }
    const uint64_t nitems = bounds.size() - 1, T = bounds.back();
    const int32_t win[][4] = {{0, W, 0, H}, {0, 1, 0, H}, {W - 1, W, 0, 1}, {0, W < 63 ? W : 63, 0, H}, {1, W < 64 ? W : 64, 0, H / 2 + 1},
                              {W > 3 ? 3 : 0, W < 67 ? W : 67, 0, H}, {0, W < 65 ? W : 65, H > 7 ? 7 : 0, H}, {W / 3, W, H / 4, H - H / 4}};
    int cases = 0;
    for (const auto &w : win) {
        const int32_t x0 = w[0], x1 = w[1], y0 = w[2], y1 = w[3];
        if (x1 <= x0 || y1 <= y0) continue;
        for (int item = 0; item < 2; ++item) {
            const uint64_t n = item ? nitems : T;
            for (const uint64_t entries : {(uint64_t)0, (uint64_t)1, n / 2, n, n + 9}) {
                std::vector<uint32_t> got(entries, 0xDEADBEEFu), want(entries, 0u);   // (exactly `entries`: a write past the end is the sanitizer's to find)
                frr::visible_counts_host(ids.data(), x0, x1, y0, y1, item ? bounds.data() : nullptr, n, got.data(), entries);
                for (int32_t ry = 0; ry < y1 - y0; ++ry)
                    for (int32_t c = 0; c < x1 - x0; ++c) {
                        const uint32_t id = ids[(size_t)ry * (size_t)x1 + (size_t)c];
                        if (id == 0xFFFFFFFFu) continue;
                        uint64_t u = id;
                        if (item) {
                            if (id < bounds[0] || id >= bounds[nitems]) continue;
                            u = 0;
                            while (!(bounds[u] <= id && id < bounds[u + 1])) ++u;
                        }
                        if (u < n && u < entries) ++want[u];
                    }
                if (got != want) { std::printf("visible_host: MISMATCH window %d %d %d %d item %d entries %llu\n", x0, x1, y0, y1, item, (unsigned long long)entries); return 1; }
                ++cases;
            }
        }
    }
    std::printf("visible_host: ok %d\n", cases);
    return 0;
}
