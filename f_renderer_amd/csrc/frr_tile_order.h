// frr_tile_order.h -- host side of option tile_order: when may a raster pass order its tile kernel's blocks by the costs
// an earlier pass recorded (frr_kernels.h: build_tile_perm)?  Plain C++ (no HIP), so that a CPU test can hold the rule.
//
// A workspace set (BinSet) keeps one cost per tile, written by every tile kernel of the segmented path that uses the set,
// and the key of the pass that wrote it.  A later pass on the same set orders its tiles by those costs only if its own key
// is the same: the same grid of tiles (window, partition) and the same workgroup shape.  The order never changes a
// result (tiles are independent, and the order is a permutation whatever the costs hold); the rule is about costs that
// fit the tiles they are applied to.
#pragma once
#include <stdint.h>

namespace frr {

enum TileOrder { TILE_ORDER_FIXED = 0, TILE_ORDER_HEAVY_FIRST = 1, TILE_ORDER_RANDOM = 2 };

// Heavy first is only tried where the tiles take about two rounds of the chip's workgroup slots (1,536 four-wave tiles),
// as on the 1080p frame's 2,040; it did not shorten that frame's tile kernel either.  With many
// rounds (8,122 and 15,372 tiles: 4K, 4096^2) it measured no faster, and sorting that many tiles in one workgroup
// lengthened the binning launch (25 -> 46 us on 4096^2): larger grids always keep the fixed order.
constexpr uint32_t TILE_ORDER_MAX_TILES = 4096;

struct TileOrderKey {
    uint32_t grid;                    // the rank's tiles (blocks of the tile kernel)
    int32_t tiles_x, x0, x1, y0, y1;  // window
    int32_t rank, world, blocked;     // tile-row ownership
    int32_t nw;                       // waves per tile workgroup (what a tile costs depends on it)
};

inline bool same_tile_order_key(const TileOrderKey &a, const TileOrderKey &b)
{
    return a.grid == b.grid && a.tiles_x == b.tiles_x && a.x0 == b.x0 && a.x1 == b.x1 && a.y0 == b.y0 && a.y1 == b.y1 &&
           a.rank == b.rank && a.world == b.world && a.blocked == b.blocked && a.nw == b.nw;
}

// Does the pass with key `cur` take a built order?  `have_prev`: the set holds costs, written under `prev`.  A replay
// (after a list overflowed) keeps the fixed order.
inline bool tile_order_built(int order, bool replay, const TileOrderKey &cur, bool have_prev, const TileOrderKey &prev)
{
    if (order == TILE_ORDER_FIXED || replay || cur.grid == 0u) return false;
    if (order == TILE_ORDER_RANDOM) return true;   // (needs no history)
    return cur.grid <= TILE_ORDER_MAX_TILES && have_prev && same_tile_order_key(prev, cur);
}

} // namespace frr
