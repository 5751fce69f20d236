// craft_tick_lang.hip — craft_step_lang: one tick of the language trainers' rollout protocol
// (trainers/primitive_language.py:45-66 and its interactive / active variants), the tile
// kernel's MODE_LANG (craft_tile.h): every running env steps first, then the timer drops and
// done latches, and satisfies() is read off the new state.  With a label buffer the
// DemonstrationTeacher runs beside the observation stores exactly as in craft_step_teach's
// one-tile kernel (the same tiles, teacher lanes and cell-set words); without one the launch
// has the bare tick's shape.
#include "craft_tile.h"

namespace craft {

template <int WIN, int TILE>
static hipError_t launch_bare(const SimView& v, const TileArgs& a, size_t lds, hipStream_t st) {
  const int64_t tiles = (a.n + TILE - 1) / TILE;
  if (tiles == 0) return hipSuccess;
  const hipError_t e = ensure_lds<&tile_kernel<WIN, MODE_LANG, TILE>>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((tile_kernel<WIN, MODE_LANG, TILE>), dim3((unsigned)tiles), dim3(kThreads), lds, st, v, a);
  return hipGetLastError();
}

template <int TILE>
static hipError_t launch_bare_win(int win, const SimView& v, const TileArgs& a, size_t lds, hipStream_t st) {
  switch (win) {
    case 3: return launch_bare<3, TILE>(v, a, lds, st);
    case 5: return launch_bare<5, TILE>(v, a, lds, st);
    default: return launch_bare<7, TILE>(v, a, lds, st);
  }
}

template <int WIN, int TL, int NW, int TILE>
static hipError_t launch_lt(const SimView& v, const TileArgs& a, size_t lds, hipStream_t st) {
  const int64_t tiles = (a.n + TILE - 1) / TILE;
  if (tiles == 0) return hipSuccess;
  const hipError_t e = ensure_lds<&tile_kernel<WIN, MODE_LANG, TILE, TL, NW>>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((tile_kernel<WIN, MODE_LANG, TILE, TL, NW>), dim3((unsigned)tiles),
                     dim3(tile_tick_threads(TILE, TL) + TILE * TL), lds, st, v, a);
  return hipGetLastError();
}

// 3x3 windows: 64-env tiles; wider ones 32 (the handle's default tile) or 64
template <int TL, int NW>
static hipError_t launch_lt_win(int win, int tile, const SimView& v, const TileArgs& a, size_t lds, hipStream_t st) {
  switch (win) {
    case 3: return launch_lt<3, TL, NW, kMaxTileEnvs>(v, a, lds, st);
    case 5: return tile == 32 ? launch_lt<5, TL, NW, 32>(v, a, lds, st) : launch_lt<5, TL, NW, kMaxTileEnvs>(v, a, lds, st);
    default: return tile == 32 ? launch_lt<7, TL, NW, 32>(v, a, lds, st) : launch_lt<7, TL, NW, kMaxTileEnvs>(v, a, lds, st);
  }
}

template <int TL>
static hipError_t launch_lt_nw(int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds, hipStream_t st) {
  // nw rounded up to an instantiated NW, as launch_tick_teach does
  if (nw <= 2) return launch_lt_win<TL, 2>(win, tile, v, a, lds, st);
  if (nw <= 4) return launch_lt_win<TL, 4>(win, tile, v, a, lds, st);
  if (nw <= 5) return launch_lt_win<TL, 5>(win, tile, v, a, lds, st);
  return launch_lt_win<TL, 8>(win, tile, v, a, lds, st);
}

// tl = teacher lanes per env (1, 2 or 4), or 0: no teacher in the launch (tile 16, 32 or 64).
hipError_t launch_tick_lang(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                            hipStream_t st) {
  if (tl == 0) {
    switch (tile) {
      case 16: return launch_bare_win<16>(win, v, a, lds, st);
      case 32: return launch_bare_win<32>(win, v, a, lds, st);
      default: return launch_bare_win<64>(win, v, a, lds, st);
    }
  }
  if (tl == 1) return launch_lt_nw<1>(nw, win, tile, v, a, lds, st);
  if (tl == 4) return launch_lt_nw<4>(nw, win, tile, v, a, lds, st);
  return launch_lt_nw<2>(nw, win, tile, v, a, lds, st);
}

}  // namespace craft
