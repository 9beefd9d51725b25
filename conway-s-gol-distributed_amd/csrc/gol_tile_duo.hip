// gol_tile_duo.hip -- the k_step_tile_duo instantiation table (K1t with the interior rows ruled
// in pairs on shared row-pair sums: gol_tile.h, tile_pass DUO).  Its own unit, so these kernels
// compile beside gol_tile.hip's.
#include "gol_tile.h"

namespace golk {

void *tile_duo_kernel(int code)
{
    switch (code) {
    case 516: return reinterpret_cast<void *>(&k_step_tile_duo<16, 5, 1>);
    default: return nullptr;
    }
}

}  // namespace golk
