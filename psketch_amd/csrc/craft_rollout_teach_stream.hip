// craft_rollout_teach_stream.hip — craft_rollout_teach_stream: rollout_teach_kernel's QUEUE
// instantiations (craft_rollout_teach.h), the teacher-labelled K-tick launch on the episode
// queue.  The launch shape is craft_rollout_teach's: 512 threads on rt_tile(window) envs, one work
// unit per tile for the whole launch, one instantiation per window, BFS word count and label
// source.  A translation unit of its own, so that the craft_rollout_teach kernels' unit compiles
// as before.
#include <algorithm>

#include "craft_launch.h"
#include "craft_rollout_teach.h"

namespace craft {
namespace {

template <int WIN, int NW, bool LA>
hipError_t launch_one(const SimView& v, const RolloutArgs& a, hipStream_t st) {
  constexpr int TILE = rt_tile(WIN);
  const int64_t tiles = (v.n_envs + TILE - 1) / TILE;
  if (tiles == 0 || a.n_ticks == 0) return hipSuccess;
  const size_t lds = (size_t)rt_lds(TILE, v.GS, v.F, NW, true).bytes;
  constexpr auto kern = &rollout_teach_kernel<WIN, TILE, NW, LA, true>;
  {
    const hipError_t e = ensure_lds<kern>(lds);
    if (e != hipSuccess) return e;
  }
  // persistent workgroups, every one the same number of tiles (craft_rollout_teach.hip)
  const int resident = resident_workgroups<kern>(kRtThreads, lds);
  const int64_t rounds = (tiles + resident - 1) / resident;
  const int64_t rows = (v.n_envs + kMinTileEnvs - 1) / kMinTileEnvs;   // stats_part rows
  const int64_t grid = std::min<int64_t>((tiles + rounds - 1) / rounds, rows);
  if (a.grid_out) *a.grid_out = grid;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kRtThreads), lds, st, v, a);
  return hipGetLastError();
}

template <int WIN, bool LA>
hipError_t launch_nw(int nw, const SimView& v, const RolloutArgs& a, hipStream_t st) {
  if (nw <= 2) return launch_one<WIN, 2, LA>(v, a, st);
  if (nw <= 4) return launch_one<WIN, 4, LA>(v, a, st);
  return launch_one<WIN, 8, LA>(v, a, st);
}

template <int WIN>
hipError_t launch_win(int nw, const SimView& v, const RolloutArgs& a, hipStream_t st) {
  // labels feeding actions, the transition wave looking them up (lsync 2): the LA kernel
  if (a.lsync == 2) return launch_nw<WIN, true>(nw, v, a, st);
  return launch_nw<WIN, false>(nw, v, a, st);
}

}  // namespace

hipError_t launch_rollout_teach_stream(int win, int nw, const SimView& v, const RolloutArgs& a, hipStream_t st) {
  switch (win) {
    case 3: return launch_win<3>(nw, v, a, st);
    case 5: return launch_win<5>(nw, v, a, st);
    default: return launch_win<7>(nw, v, a, st);
  }
}

}  // namespace craft
