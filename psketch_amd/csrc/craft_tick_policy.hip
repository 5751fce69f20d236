// craft_tick_policy.hip — the policy head (include/craft.h "The head rule", craft_policy.h):
// craft_policy_actions' and craft_policy_ask's kernels, one thread per slot, and the tile kernel's MODE_TICK_HEAD
// instantiations that craft_step_policy launches (the shapes of craft_step_ex and of
// craft_step_teach's one-tile kernel; the two-tile kernel's twin is in craft_tick_teach.hip).
#include "craft_launch.h"
#include "craft_tile_launch.h"

namespace craft {

__global__ __launch_bounds__(256) void policy_actions_kernel(const float* logits, int32_t mode, uint64_t seed,
                                                              int64_t gid0, int64_t tick, int64_t n,
                                                              int32_t* actions_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const LogitRow row = load_logit_row(logits, i);
  actions_out[i] = policy_head(row, mode, seed, (uint64_t)(gid0 + i), tick);
}

hipError_t launch_policy_actions(const float* logits, int32_t mode, uint64_t seed, int64_t gid0, int64_t tick,
                                 int64_t n, int32_t* actions_out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(policy_actions_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, logits, mode, seed,
                     gid0, tick, n, actions_out);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void policy_ask_kernel(const float* logits, float threshold, int64_t n,
                                                          uint8_t* ask_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const LogitRow row = load_logit_row(logits, i);
  ask_out[i] = (uint8_t)policy_ask(row, threshold);
}

hipError_t launch_policy_ask(const float* logits, float threshold, int64_t n, uint8_t* ask_out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(policy_ask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, logits, threshold, n,
                     ask_out);
  return hipGetLastError();
}

hipError_t launch_tick_head(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                            hipStream_t st) {
  if (tl == 0) return launch_tile_bare<MODE_TICK_HEAD>(win, tile, v, a, lds, st);
  return launch_tile_teach<MODE_TICK_HEAD>(tl, nw, win, tile, v, a, lds, st);
}

}  // namespace craft
