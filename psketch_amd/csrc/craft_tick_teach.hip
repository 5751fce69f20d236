// craft_tick_teach.hip — craft_step_teach: one rollout tick fused with the
// DemonstrationTeacher on every env's new state (config 5: a DAgger label per
// tick).  The tile kernel (craft_tile.h) with TILE * TL teacher threads beside
// its 256: the tick's waves stream the observations while the teacher waves run
// teach_env on the grid rows the tick left in LDS, so the teacher reads no grid
// from HBM and needs no launch of its own.  For 3x3 windows the two-tile tick
// kernel (craft_tick2.h) serves craft_step_teach.
#include "craft_launch.h"
#include "craft_tick2.h"
#include "craft_tile_launch.h"

namespace craft {

// head (here and in launch_tick2): the policy head's instantiations (a.logits set)
hipError_t launch_tick_teach(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                             hipStream_t st, bool head) {
  if (head) return launch_tick_head(tl, nw, win, tile, v, a, lds, st);             // (craft_tick_policy.hip)
  return launch_tile_teach<MODE_TICK>(tl, nw, win, tile, v, a, lds, st);
}

// The two-tile tick kernel (craft_tick2.h) for craft_step_teach, 3x3 windows: 2 or 4 teacher
// lanes per env, 4 tick waves (8 would leave the BFS too few registers at 2 workgroups per CU).
constexpr int kTick2Tiles = 2, kTick2TickWaves = 4;

size_t tick2_lds_bytes(int tl, int nw, int GS, int F) {
  const int nbuf = tick2_share(tl, teach_nw(nw)) ? kTick2TickWaves + kTick2Tiles * tl : kTick2TickWaves;
  return (size_t)tick2_lds(kTick2Tiles, kTick2TickWaves, GS, F, nbuf).bytes;
}

template <auto KERNEL, int TL>
static hipError_t launch_t2(const SimView& v, const TileArgs& a, size_t lds, hipStream_t st) {
  constexpr int TW = kTick2TickWaves;
  const int64_t per = (int64_t)kTick2Tiles * kTick2Tile;
  const int64_t blocks = (a.n + per - 1) / per;
  if (blocks == 0) return hipSuccess;
  // the teacher waves' own rows (tick2_share) pass 64 KiB
  const hipError_t e = ensure_lds<KERNEL>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)blocks), dim3(64 * TW + kTick2Tiles * kTick2Tile * TL), lds, st, v, a);
  return hipGetLastError();
}

hipError_t launch_tick2(int tl, int nw, const SimView& v, const TileArgs& a, size_t lds, hipStream_t st, bool head) {
  constexpr int J = kTick2Tiles, TW = kTick2TickWaves;
  return dispatch_nw(nw, [&](auto nwc) {
    constexpr int NW = decltype(nwc)::value;
    if (head)
      return tl == 4 ? launch_t2<&tick2_kernel<3 + kTick2Head, J, TW, 4, NW>, 4>(v, a, lds, st)
                     : launch_t2<&tick2_kernel<3 + kTick2Head, J, TW, 2, NW>, 2>(v, a, lds, st);
    return tl == 4 ? launch_t2<&tick2_kernel<3, J, TW, 4, NW>, 4>(v, a, lds, st)
                   : launch_t2<&tick2_kernel<3, J, TW, 2, NW>, 2>(v, a, lds, st);
  });
}

}  // namespace craft
