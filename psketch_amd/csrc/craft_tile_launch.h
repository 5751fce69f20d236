// craft_tile_launch.h — the launch ladder of the tile kernel (craft_tile.h), templated on MODE:
// launch_tile_bare (no teacher: 256 threads per tile of 16, 32 or 64 envs) and launch_tile_teach
// (TILE * TL teacher threads beside the tick's, craft_step_teach's one-tile shapes).  Each .hip
// file instantiates the modes it owns, so the kernels stay spread over the translation units.
#pragma once
#include "craft_tile.h"

namespace craft {

// tile_kernel<WIN, MODE, TILE> is tile_kernel<WIN, MODE, TILE, 0, 0>: TL = 0 is the bare launch.
template <int WIN, int MODE, int TILE, int TL = 0, int NW = 0>
static hipError_t launch_tile_one(const SimView& v, const TileArgs& a, size_t lds, hipStream_t st) {
  const int64_t tiles = (a.n + TILE - 1) / TILE;
  if (tiles == 0) return hipSuccess;
  // u8 rows of 5x5 / 7x7 windows on large tiles: rows past 64 KiB
  const hipError_t e = ensure_lds<&tile_kernel<WIN, MODE, TILE, TL, NW>>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((tile_kernel<WIN, MODE, TILE, TL, NW>), dim3((unsigned)tiles),
                     dim3(tile_tick_threads(TILE, TL) + TILE * TL), lds, st, v, a);
  return hipGetLastError();
}

template <int MODE, int TILE>
static hipError_t launch_tile_bare_win(int win, const SimView& v, const TileArgs& a, size_t lds, hipStream_t st) {
  switch (win) {
    case 3: return launch_tile_one<3, MODE, TILE>(v, a, lds, st);
    case 5: return launch_tile_one<5, MODE, TILE>(v, a, lds, st);
    default: return launch_tile_one<7, MODE, TILE>(v, a, lds, st);
  }
}

template <int MODE>
static hipError_t launch_tile_bare(int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                                   hipStream_t st) {
  switch (tile) {
    case 16: return launch_tile_bare_win<MODE, 16>(win, v, a, lds, st);
    case 32: return launch_tile_bare_win<MODE, 32>(win, v, a, lds, st);
    default: return launch_tile_bare_win<MODE, 64>(win, v, a, lds, st);
  }
}

// 3x3 windows: 64-env tiles; wider ones 32 (the handle's default tile) or 64
template <int MODE, int TL, int NW>
static hipError_t launch_tile_teach_win(int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                                        hipStream_t st) {
  switch (win) {
    case 3: return launch_tile_one<3, MODE, kMaxTileEnvs, TL, NW>(v, a, lds, st);
    case 5: return tile == 32 ? launch_tile_one<5, MODE, 32, TL, NW>(v, a, lds, st)
                              : launch_tile_one<5, MODE, kMaxTileEnvs, TL, NW>(v, a, lds, st);
    default: return tile == 32 ? launch_tile_one<7, MODE, 32, TL, NW>(v, a, lds, st)
                               : launch_tile_one<7, MODE, kMaxTileEnvs, TL, NW>(v, a, lds, st);
  }
}

// tl = teacher lanes per env: 2 (a pair per env, 2 teacher waves), 4 (a quad, 4 waves) or
// 1 (one wave); nw = 32-bit words per BFS cell set (dispatch_nw, craft_teach.h).
template <int MODE>
static hipError_t launch_tile_teach(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a,
                                    size_t lds, hipStream_t st) {
  return dispatch_nw(nw, [&](auto nwc) {
    constexpr int NW = decltype(nwc)::value;
    if (tl == 1) return launch_tile_teach_win<MODE, 1, NW>(win, tile, v, a, lds, st);
    if (tl == 4) return launch_tile_teach_win<MODE, 4, NW>(win, tile, v, a, lds, st);
    return launch_tile_teach_win<MODE, 2, NW>(win, tile, v, a, lds, st);
  });
}

}  // namespace craft
