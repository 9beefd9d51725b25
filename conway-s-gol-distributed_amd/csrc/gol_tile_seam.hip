// gol_tile_seam.hip -- the k_step_tile_seam instantiation table (K1t across the row seam:
// gol_tile.h, tile_pass SEAM).  Its own unit, so these kernels compile beside gol_tile.hip's.
#include "gol_tile.h"

#include <iterator>

namespace golk {

void *tile_seam_kernel(int code)
{
    static_assert(std::size(kTileSeamCodes) == 10, "tile_seam_kernel covers kTileSeamCodes");
    switch (code) {
    case 2: return reinterpret_cast<void *>(&k_step_tile_seam<2, 0>);
    case 16: return reinterpret_cast<void *>(&k_step_tile_seam<16, 0>);
    case 102: return reinterpret_cast<void *>(&k_step_tile_seam<2, 1>);
    case 104: return reinterpret_cast<void *>(&k_step_tile_seam<4, 1>);
    case 106: return reinterpret_cast<void *>(&k_step_tile_seam<6, 1>);
    case 108: return reinterpret_cast<void *>(&k_step_tile_seam<8, 1>);
    case 112: return reinterpret_cast<void *>(&k_step_tile_seam<12, 1>);
    case 116: return reinterpret_cast<void *>(&k_step_tile_seam<16, 1>);
    case 516: return reinterpret_cast<void *>(&k_step_tile_seam<16, 5>);
    case 524: return reinterpret_cast<void *>(&k_step_tile_seam<24, 5>);
    default: return nullptr;
    }
}

}  // namespace golk
