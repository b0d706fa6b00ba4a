// The depth test of frr_query_pixels (frr_rules.h: fragment_passes, the comparison its kernel runs) in a program of its
// own: tests/test_query_cpu.py builds it plain and under the address and undefined-behaviour sanitizers.  Exits 0 and
// prints "query_host: ok" only if every case holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/frr.h"
#include "../f_renderer_amd/csrc/frr_rules.h"

static float bits(uint32_t u) { float f; std::memcpy(&f, &u, sizeof f); return f; }

int main()
{
    using frr::fragment_passes;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float sub = bits(0x00000001u), sub2 = bits(0x00000002u), nsub = bits(0x80000001u);
    int bad = 0;
    auto expect = [&](float rhw, float depth, bool want) {
        if (fragment_passes(rhw, depth) != want) { std::printf("fragment_passes(%a, %a) != %d\n", rhw, depth, (int)want); ++bad; }
    };
    // ties pass, on every kind of value; +0 and -0 are a tie
    const std::vector<float> vals = {0.0f, -0.0f, 1.0f, -1.0f, 0.25f, sub, nsub, sub2, inf, -inf, 3.0e38f, -3.0e38f};
    for (float v : vals) expect(v, v, true);
    expect(0.0f, -0.0f, true); expect(-0.0f, 0.0f, true);
    // a NaN on either side passes, whatever the other side holds
    for (float v : vals) { expect(nan, v, true); expect(v, nan, true); }
    expect(nan, nan, true); expect(bits(0xFFC00000u), 1.0f, true); expect(1.0f, bits(0x7FC00001u), true);
    // otherwise the ordinary order: strictly below fails, at or above passes
    for (float a : vals) for (float b : vals) expect(a, b, !(a < b));
    expect(sub, sub2, false); expect(sub2, sub, true); expect(nsub, sub, false); expect(sub, nsub, true); expect(nsub, 0.0f, false);
    expect(-inf, inf, false); expect(inf, -inf, true); expect(3.0e38f, inf, false); expect(inf, 3.0e38f, true); expect(-inf, -3.0e38f, false);
    expect(std::nextafter(1.0f, 0.0f), 1.0f, false); expect(std::nextafter(1.0f, 2.0f), 1.0f, true);
    if (bad) return 1;
    std::printf("query_host: ok\n");
    return 0;
}
