// craft_tile.hip — launchers of the tile kernel (craft_tile.h) for the tick,
// transition, observe and reset entry points.
#include "craft_launch.h"
#include "craft_tile_launch.h"

namespace craft {

hipError_t launch_tile(int mode, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                       hipStream_t st) {
  switch (mode) {
    case MODE_TICK: return launch_tile_bare<MODE_TICK>(win, tile, v, a, lds, st);
    case MODE_TICK_HEAD: return launch_tick_head(0, 0, win, tile, v, a, lds, st);   // (craft_tick_policy.hip)
    case MODE_OBSERVE: return launch_tile_bare<MODE_OBSERVE>(win, tile, v, a, lds, st);
    case MODE_TRANSITION: return launch_tile_bare<MODE_TRANSITION>(win, tile, v, a, lds, st);
    default: return launch_tile_bare<MODE_RESET>(win, tile, v, a, lds, st);
  }
}

}  // namespace craft
