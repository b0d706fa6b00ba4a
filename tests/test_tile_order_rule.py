"""CPU: the host's rule for when a raster pass orders its tile kernel's blocks by recorded costs (option tile_order,
f_renderer_amd/csrc/frr_tile_order.h), compiled with the host compiler and run: the fixed order on the first pass, on a
replay, and whenever the grid, window, partition or workgroup shape differs from the pass that recorded the costs;
the random order needs no history."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "frr_tile_order.h"
#include <stdio.h>
using namespace frr;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); ++fails; } } while (0)
int main()
{
    const TileOrderKey k = {2040, 60, 0, 1920, 0, 1080, 0, 1, 0, 4};
    CHECK(!tile_order_built(TILE_ORDER_HEAVY_FIRST, false, k, false, k));   // first pass: nothing recorded
    CHECK(tile_order_built(TILE_ORDER_HEAVY_FIRST, false, k, true, k));     // same grid as the recording pass
    CHECK(!tile_order_built(TILE_ORDER_HEAVY_FIRST, true, k, true, k));     // replay after an overflow
    CHECK(!tile_order_built(TILE_ORDER_FIXED, false, k, true, k));
    CHECK(tile_order_built(TILE_ORDER_RANDOM, false, k, false, k));         // needs no history ...
    CHECK(!tile_order_built(TILE_ORDER_RANDOM, true, k, false, k));         // ... but not on a replay either
    TileOrderKey big = k; big.grid = TILE_ORDER_MAX_TILES + 1;             // many rounds of workgroups: not worth it ...
    CHECK(!tile_order_built(TILE_ORDER_HEAVY_FIRST, false, big, true, big));
    CHECK(tile_order_built(TILE_ORDER_RANDOM, false, big, true, big));      // ... but the random order (tests) still goes
    TileOrderKey z = k; z.grid = 0;
    CHECK(!tile_order_built(TILE_ORDER_RANDOM, false, z, true, z));         // nothing to order
    for (int f = 0; f < 10; ++f) {                                          // any field that differs: the fixed order
        TileOrderKey p = k;
        int32_t *w = f == 0 ? (int32_t *)&p.grid : f == 1 ? &p.tiles_x : f == 2 ? &p.x0 : f == 3 ? &p.x1 : f == 4 ? &p.y0 :
                     f == 5 ? &p.y1 : f == 6 ? &p.rank : f == 7 ? &p.world : f == 8 ? &p.blocked : &p.nw;
        *w += 1;
        CHECK(!same_tile_order_key(p, k));
        CHECK(!tile_order_built(TILE_ORDER_HEAVY_FIRST, false, k, true, p));
        CHECK(tile_order_built(TILE_ORDER_RANDOM, false, k, true, p));
    }
    printf("%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
"""


def test_tile_order_rule(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "rule.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rule"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "f_renderer_amd", "csrc"),
                           "-o", str(exe), str(src)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout
