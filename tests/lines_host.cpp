// lines_host.cpp -- FrameBuffer::draw_line of the C++ host mirror (f_renderer_amd/host/frr_renderer.hpp), one call at a
// time on an empty W x H FrameBuffer, for tests/test_lines_cpu.py:
//   lines_host <W> <H> <segments.u32> <out.u32>
// segments.u32: n x {x1, y1, x2, y2} u32.  out.u32, per segment: 1 if the call threw (the reference's panic) else 0, the
// number of pixels it painted, and their linear indices y * W + x in ascending order (none if it threw).
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>

#include "../f_renderer_amd/host/frr_renderer.hpp"

int main(int argc, char **argv)
{
    if (argc < 5) { std::cerr << "usage: lines_host W H segments.u32 out.u32\n"; return 2; }
    const uint32_t W = (uint32_t)std::strtoul(argv[1], nullptr, 10), H = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    std::ifstream f(argv[3], std::ios::binary);
    if (!f) { std::cerr << "cannot open " << argv[3] << "\n"; return 2; }
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const size_t n = raw.size() / 16;
    const uint32_t *seg = reinterpret_cast<const uint32_t *>(raw.data());
    std::vector<uint32_t> out;
    frr::FrameBuffer fb = frr::FrameBuffer::create(W, H);
    for (size_t k = 0; k < n; ++k) {
        bool threw = false;
        try { fb.draw_line(seg[4 * k], seg[4 * k + 1], seg[4 * k + 2], seg[4 * k + 3], {255, 255, 255, 255}); }
        catch (const std::out_of_range &) { threw = true; }
        out.push_back(threw ? 1u : 0u);
        const size_t at = out.size();
        out.push_back(0u);
        const std::vector<uint8_t> &d = fb.get_data();
        for (size_t p = 0; p < (size_t)W * H; ++p)
            if (d[p * 4 + 3]) { if (!threw) { out.push_back((uint32_t)p); ++out[at]; } }
        fb.clear();
    }
    std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), (std::streamsize)(out.size() * 4));
    return 0;
}
