// gol_tile_big.hip -- the k_step_tile_big instantiation table (K1t on a buffer of 2 GiB or more:
// gol_tile.h, tile_pass BIG).  Its own unit, so these kernels compile beside gol_tile.hip's.
#include "gol_tile.h"

#include <iterator>

namespace golk {

void *tile_big_kernel(int code)
{
    static_assert(std::size(kTileBigCodes) == 8, "tile_big_kernel covers kTileBigCodes");
    switch (code) {
    case 16: return reinterpret_cast<void *>(&k_step_tile_big<16, 0>);
    case 108: return reinterpret_cast<void *>(&k_step_tile_big<8, 1>);
    case 112: return reinterpret_cast<void *>(&k_step_tile_big<12, 1>);
    case 116: return reinterpret_cast<void *>(&k_step_tile_big<16, 1>);
    case 512: return reinterpret_cast<void *>(&k_step_tile_big<12, 5>);
    case 516: return reinterpret_cast<void *>(&k_step_tile_big<16, 5>);
    case 524: return reinterpret_cast<void *>(&k_step_tile_big<24, 5>);
    case 616: return reinterpret_cast<void *>(&k_step_tile_big<16, 6>);
    default: return nullptr;
    }
}

}  // namespace golk
