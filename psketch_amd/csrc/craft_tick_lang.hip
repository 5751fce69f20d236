// craft_tick_lang.hip — craft_step_lang: one tick of the language trainers' rollout protocol
// (trainers/primitive_language.py:45-66 and its interactive / active variants), the tile
// kernel's MODE_LANG (craft_tile.h): every running env steps first, then the timer drops and
// done latches, and satisfies() is read off the new state.  With a label buffer the
// DemonstrationTeacher runs beside the observation stores exactly as in craft_step_teach's
// one-tile kernel (the same tiles, teacher lanes and cell-set words); without one the launch
// has the bare tick's shape.
#include "craft_launch.h"
#include "craft_tile_launch.h"

namespace craft {

// tl = teacher lanes per env (1, 2 or 4), or 0: no teacher in the launch (tile 16, 32 or 64).
// head: the policy head's instantiations (a.logits set; craft_tick_lang_policy.hip).
hipError_t launch_tick_lang(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                            hipStream_t st, bool head) {
  if (head) return launch_tick_lang_head(tl, nw, win, tile, v, a, lds, st);
  if (tl == 0) return launch_tile_bare<MODE_LANG>(win, tile, v, a, lds, st);
  return launch_tile_teach<MODE_LANG>(tl, nw, win, tile, v, a, lds, st);
}

}  // namespace craft
