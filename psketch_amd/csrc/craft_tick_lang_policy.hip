// craft_tick_lang_policy.hip — craft_step_lang_policy: the tile kernel's MODE_LANG_HEAD
// instantiations, craft_step_lang's shapes (craft_tick_lang.hip) with the action chosen by the
// policy head (craft_policy.h) of the slot's main row or, where use_alt is set and a second head
// is given, of its alt row.  A translation unit of its own, like the other tick modes'.
#include "craft_launch.h"
#include "craft_tile_launch.h"

namespace craft {

hipError_t launch_tick_lang_head(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                                 hipStream_t st) {
  if (tl == 0) return launch_tile_bare<MODE_LANG_HEAD>(win, tile, v, a, lds, st);
  return launch_tile_teach<MODE_LANG_HEAD>(tl, nw, win, tile, v, a, lds, st);
}

}  // namespace craft
