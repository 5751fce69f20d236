// craft_rollout_replay.hip — craft_episode_actions and craft_rollout_replay: the kernel that
// checks and packs the recorded action sequences of a queue (the tape), and
// rollout_split_kernel's TAPE instantiations (craft_rollout_split.h), craft_rollout_stream's
// launch whose producer wave reads its own actions.  The shapes are craft_rollout_stream.hip's:
// 512 threads on 32- or 16-env tiles, one work unit per tile for the whole launch, every obs
// format.  A translation unit of its own, so that the other rollout kernels' units compile as
// before.
#include "craft_launch.h"
#include "craft_rollout.h"

namespace craft {
namespace {

// One thread per queue entry: its row of T int32 (actions, then -1) checked and packed into
// `stride` bytes (stride >= T, a multiple of 4), padded with STOP, and the lowest invalid index.
// Valid: 1..T values in 0..5 followed only by -1, ending in its only STOP or T long.
__global__ void tape_pack_kernel(const int32_t* actions, int64_t count, int T, int stride, uint8_t* out,
                                 unsigned long long* first_bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int32_t* row = actions + i * T;
  uint32_t* dst = reinterpret_cast<uint32_t*>(out + i * stride);
  int len = 0;                                            // actions before the first -1
  bool ok = true;
  for (int w = 0; w < stride; w += 4) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int p = w + b;
      int a = CRAFT_STOP;
      if (p < T) {
        const int x = row[p];
        if (x == -1) {
          // padding: reads as STOP
        } else if (x < 0 || x >= CRAFT_N_ACTIONS || len != p || (p > 0 && row[p - 1] == CRAFT_STOP)) {
          ok = false;                                     // out of range, after a -1, or after a STOP
        } else {
          a = x;
          len = p + 1;
        }
      }
      word |= (uint32_t)a << (8 * b);
    }
    dst[w >> 2] = word;
  }
  if (ok && (len == 0 || (len < T && row[len - 1] != CRAFT_STOP))) ok = false;   // empty, or short without a STOP
  if (!ok) atomicMin(first_bad, (unsigned long long)i);
}

template <int WIN, int TILE, int FMT>
hipError_t launch_one(const SimView& v, const RolloutArgs& a, hipStream_t st) {
  constexpr int NT = 512;
  constexpr int WPE = WIN == 3 ? CRAFT_SPLIT_WPE : 2;
  const int64_t tiles = (v.n_envs + TILE - 1) / TILE;
  if (a.n_ticks == 0) return hipSuccess;
  const size_t lds = (size_t)split_lds_bytes(TILE, v.GS, v.F, v.CS, false);
  return launch_persistent<&rollout_split_kernel<WIN, TILE, NT, FMT, WPE, false, false, true, true>>(NT, lds, tiles, v, a, st);
}

template <int WIN>
hipError_t launch_win(int tile, const SimView& v, const RolloutArgs& a, hipStream_t st) {
  auto with_fmt = [&](auto fmt) {
    return tile == 16 ? launch_one<WIN, 16, decltype(fmt)::value>(v, a, st)
                      : launch_one<WIN, 32, decltype(fmt)::value>(v, a, st);
  };
  switch (v.obs_fmt) {
    case CRAFT_OBS_BF16: return with_fmt(std::integral_constant<int, CRAFT_OBS_BF16>{});
    case CRAFT_OBS_U8: return with_fmt(std::integral_constant<int, CRAFT_OBS_U8>{});
    default: return with_fmt(std::integral_constant<int, CRAFT_OBS_F32>{});
  }
}

}  // namespace

hipError_t launch_tape_pack(const int32_t* actions, int64_t count, int T, int stride, uint8_t* out,
                            unsigned long long* first_bad, hipStream_t st) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(tape_pack_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, actions, count, T,
                     stride, out, first_bad);
  return hipGetLastError();
}

// the tile is rollout_stream_tile's (craft_rollout_stream.hip)
hipError_t launch_rollout_replay(int win, int tile, const SimView& v, const RolloutArgs& a, hipStream_t st) {
  switch (win) {
    case 3: return launch_win<3>(tile, v, a, st);
    case 5: return launch_win<5>(tile, v, a, st);
    default: return launch_win<7>(tile, v, a, st);
  }
}

}  // namespace craft
