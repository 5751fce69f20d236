// craft_rollout_stream.hip — craft_rollout_stream: rollout_split_kernel's QUEUE instantiations
// (craft_rollout_split.h), the K-tick launch on the episode queue.  One shape per window: 512
// threads on 32- or 16-env tiles, one work unit per tile for the whole launch; every obs format,
// given and hashed actions.  A translation unit of its own, so that the craft_rollout kernels'
// units compile as before.
#include "craft_launch.h"
#include "craft_rollout.h"

namespace craft {
namespace {

template <int WIN, int TILE, int FMT, bool GIVEN>
hipError_t launch_one(const SimView& v, const RolloutArgs& a, hipStream_t st) {
  constexpr int NT = 512;
  constexpr int WPE = WIN == 3 ? CRAFT_SPLIT_WPE : 2;
  const int64_t tiles = (v.n_envs + TILE - 1) / TILE;
  if (a.n_ticks == 0) return hipSuccess;
  const size_t lds = (size_t)split_lds_bytes(TILE, v.GS, v.F, v.CS, false);
  return launch_persistent<&rollout_split_kernel<WIN, TILE, NT, FMT, WPE, GIVEN, false, true>>(NT, lds, tiles, v, a, st);
}

template <int WIN>
hipError_t launch_win(int tile, const SimView& v, const RolloutArgs& a, hipStream_t st) {
  return dispatch_fmt_given(v, a, [&](auto fmt, auto given) {
    return tile == 16 ? launch_one<WIN, 16, decltype(fmt)::value, decltype(given)::value>(v, a, st)
                      : launch_one<WIN, 32, decltype(fmt)::value, decltype(given)::value>(v, a, st);
  });
}

}  // namespace

// 32-env tiles; 16 where craft_sim_tune's tile is 16 or where 32 envs' two staged observation
// buffers exceed a workgroup's 160 KiB of LDS (the largest tile that fits)
int rollout_stream_tile(int tile_knob, const SimView& v) {
  return tile_knob == 16 || split_lds_bytes(32, v.GS, v.F, v.CS, false) > 163840 ? 16 : 32;
}

hipError_t launch_rollout_stream(int win, int tile, const SimView& v, const RolloutArgs& a, hipStream_t st) {
  switch (win) {
    case 3: return launch_win<3>(tile, v, a, st);
    case 5: return launch_win<5>(tile, v, a, st);
    default: return launch_win<7>(tile, v, a, st);
  }
}

}  // namespace craft
