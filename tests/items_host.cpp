// items_host.cpp -- the per-entry item lookup of frr_shade_items (f_renderer_amd/csrc/frr_visible.h: entry_items_host, which
// compiles with no HIP) in a program of its own, for tests/test_shade_items_cpu.py to build under the host sanitizers:
//   items_host <W> <H> <ids.u32> <bounds.u32>
// ids.u32: W x H triangle ids; bounds.u32: nitems + 1 item boundaries, nitems >= 1.  Over the full window and a set of
// sub-windows it compares entry_items_host with the definition taken one entry at a time (a linear scan of the boundaries)
// and its return value with the distinct items of every 64-entry span counted naively, prints "items_host: ok <cases>" and
// exits 0 only if everything agrees.  The output array is exactly as long as the window needs.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <set>
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
    if (argc < 5) { std::cerr << "usage: items_host W H ids.u32 bounds.u32\n"; return 2; }
    const int32_t W = (int32_t)std::strtol(argv[1], nullptr, 10), H = (int32_t)std::strtol(argv[2], nullptr, 10);
    const std::vector<uint32_t> ids = read_u32(argv[3]), bounds = read_u32(argv[4]);
    if (W < 1 || H < 1 || ids.size() != (size_t)W * (size_t)H || bounds.size() < 2) { std::cerr << "bad input\n"; return 2; }
    const uint32_t nitems = (uint32_t)(bounds.size() - 1);
    const int32_t win[][4] = {{0, W, 0, H}, {0, 1, 0, H}, {W - 1, W, 0, 1}, {0, W < 63 ? W : 63, 0, H}, {1, W < 64 ? W : 64, 0, H / 2 + 1},
                              {W > 3 ? 3 : 0, W < 67 ? W : 67, 0, H}, {0, W < 65 ? W : 65, H > 7 ? 7 : 0, H}, {17, W < 117 ? W : 117, 0, H},
                              {W / 3, W, H / 4, H - H / 4}};
    int cases = 0;
    for (const auto &w : win) {
        const int32_t x0 = w[0], x1 = w[1], y0 = w[2], y1 = w[3];
        if (x1 <= x0 || y1 <= y0) continue;
        const size_t last = (size_t)(y1 - y0 - 1) * (size_t)x1 + (size_t)(x1 - x0);   // the last entry the window addresses, + 1
        if (last > ids.size()) continue;
        std::vector<uint32_t> got(last, 0xDEADBEEFu), want(last, 0xDEADBEEFu);   // (exactly `last`: a write past the end is the sanitizer's to find)
        const uint64_t rounds = frr::entry_items_host(ids.data(), x0, x1, y0, y1, bounds.data(), nitems, got.data());
        uint64_t want_rounds = 0;
        for (int32_t ry = 0; ry < y1 - y0; ++ry) {
            std::set<uint32_t> span;
            for (int32_t c = 0; c < x1 - x0; ++c) {
                if (c % 64 == 0) { want_rounds += span.size(); span.clear(); }
                const size_t i = (size_t)ry * (size_t)x1 + (size_t)c;
                const uint32_t id = ids[i];
                uint32_t u = 0xFFFFFFFFu;
                if (id != 0xFFFFFFFFu && id >= bounds[0] && id < bounds[nitems]) {
                    u = 0;
                    while (!(bounds[u] <= id && id < bounds[u + 1])) ++u;
                    span.insert(u);
                }
                want[i] = u;
            }
            want_rounds += span.size();
        }
        if (got != want || rounds != want_rounds) {
            std::printf("items_host: MISMATCH window %d %d %d %d rounds %llu want %llu\n", x0, x1, y0, y1, (unsigned long long)rounds, (unsigned long long)want_rounds);
            return 1;
        }
        ++cases;
    }
    std::printf("items_host: ok %d\n", cases);
    return 0;
}
