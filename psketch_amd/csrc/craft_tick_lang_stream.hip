// craft_tick_lang_stream.hip — craft_step_lang_stream: the language trainers' tick
// (craft_tick_lang.hip) on the episode queue (craft_tick_stream.hip), the tile kernel's
// MODE_LANG_STREAM (craft_tile.h): every running env steps first, the ending tick included, then
// the timer drops, satisfies() is read off the state that step left, and only then a slot whose
// episode ended restarts on its next queue entry.  The launch shapes are craft_tick_lang.hip's:
// with a label buffer the one-tile teacher shapes, without one the bare tick's.
#include "craft_launch.h"
#include "craft_tile_launch.h"

namespace craft {

// tl = teacher lanes per env (1, 2 or 4), or 0: no teacher in the launch (tile 16, 32 or 64).
// head: the policy head's instantiations (a.logits set; craft_tick_lang_policy_stream.hip).
hipError_t launch_tick_lang_stream(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                                   hipStream_t st, bool head) {
  if (head) return launch_tick_lang_stream_head(tl, nw, win, tile, v, a, lds, st);
  if (tl == 0) return launch_tile_bare<MODE_LANG_STREAM>(win, tile, v, a, lds, st);
  return launch_tile_teach<MODE_LANG_STREAM>(tl, nw, win, tile, v, a, lds, st);
}

}  // namespace craft
