// craft_tick_lang_policy_stream.hip — craft_step_lang_policy_stream: the tile kernel's
// MODE_LANG_STREAM_HEAD instantiations, craft_step_lang_stream's shapes (craft_tick_lang_stream.hip)
// with the action chosen by the policy head (craft_policy.h) as in craft_tick_lang_policy.hip.
#include "craft_launch.h"
#include "craft_tile_launch.h"

namespace craft {

hipError_t launch_tick_lang_stream_head(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a,
                                        size_t lds, hipStream_t st) {
  if (tl == 0) return launch_tile_bare<MODE_LANG_STREAM_HEAD>(win, tile, v, a, lds, st);
  return launch_tile_teach<MODE_LANG_STREAM_HEAD>(tl, nw, win, tile, v, a, lds, st);
}

}  // namespace craft
