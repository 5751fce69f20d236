// craft_tick_policy_stream.hip — craft_step_policy_stream: the tile kernel's MODE_STREAM_HEAD
// instantiations, craft_step_stream's shapes with the action chosen by the policy head
// (craft_policy.h).  A translation unit of its own, like the other tick modes'.
#include "craft_launch.h"
#include "craft_tile_launch.h"

namespace craft {

hipError_t launch_tick_stream_head(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a,
                                   size_t lds, hipStream_t st) {
  if (tl == 0) return launch_tile_bare<MODE_STREAM_HEAD>(win, tile, v, a, lds, st);
  return launch_tile_teach<MODE_STREAM_HEAD>(tl, nw, win, tile, v, a, lds, st);
}

}  // namespace craft
