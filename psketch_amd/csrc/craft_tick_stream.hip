// craft_tick_stream.hip — the episode queue (include/craft.h craft_episode_queue,
// craft_episode_begin, craft_step_stream): the kernels that check and pack a queue and put every
// slot on its first entry, and the tile kernel's MODE_STREAM (craft_tile.h), the imitation
// trainer's tick whose auto-reset moves a finished slot onto its next queue entry.  The launch
// shapes are craft_tick_lang.hip's: with a label buffer the one-tile teacher shapes (the same
// tiles, teacher lanes and cell-set words), without one the bare tick's.
#include "craft_launch.h"
#include "craft_tile_launch.h"

namespace craft {

// One thread per queue entry: the checks craft_reset makes of a spec, the packed entry
// (.x = scenario | task << 24, .y = x | y << 8 | dir << 16), and the lowest invalid index.
__global__ void queue_pack_kernel(SimView v, const int32_t* specs, int64_t count, uint2* out,
                                  unsigned long long* first_bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int sc = specs[5 * i], x0 = specs[5 * i + 1], y0 = specs[5 * i + 2], d0 = specs[5 * i + 3],
            tk = specs[5 * i + 4];
  if (sc < 0 || sc >= v.pool_count || x0 < 1 || x0 > v.W - 2 || y0 < 1 || y0 > v.H - 2 || d0 < 0 || d0 > 3 ||
      tk < 0 || tk >= v.n_tasks) {
    atomicMin(first_bad, (unsigned long long)i);
    out[i] = make_uint2(0u, 0u);
    return;
  }
  out[i] = make_uint2((uint32_t)sc | ((uint32_t)tk << 24), (uint32_t)x0 | ((uint32_t)y0 << 8) | ((uint32_t)d0 << 16));
}

// One thread per slot: its first queue index (first + global id, mod count under wrap; the host
// has checked that it exists), as the slot's cursor and, unpacked into r[5][n], as craft_reset's
// five input arrays.
__global__ void queue_begin_kernel(const uint2* entries, int64_t count, int64_t first_gid, int wrap, int64_t n,
                                   int32_t* cursor, int32_t* r) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t q = first_gid + i;
  if (wrap) q %= count;
  const uint2 e = entries[q];
  cursor[i] = (int32_t)q;
  r[i] = (int32_t)(e.x & 0xffffffu);
  r[n + i] = (int32_t)(e.y & 0xffu);
  r[2 * n + i] = (int32_t)((e.y >> 8) & 0xffu);
  r[3 * n + i] = (int32_t)((e.y >> 16) & 3u);
  r[4 * n + i] = (int32_t)(e.x >> 24);
}

hipError_t launch_queue_pack(const SimView& v, const int32_t* specs, int64_t count, uint2* out,
                             unsigned long long* first_bad, hipStream_t st) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(queue_pack_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, v, specs, count, out,
                     first_bad);
  return hipGetLastError();
}

hipError_t launch_queue_begin(const uint2* entries, int64_t count, int64_t first_gid, int wrap, int64_t n,
                              int32_t* cursor, int32_t* r, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(queue_begin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, entries, count, first_gid,
                     wrap, n, cursor, r);
  return hipGetLastError();
}

// tl = teacher lanes per env (1, 2 or 4), or 0: no teacher in the launch (tile 16, 32 or 64).
// head: the policy head's instantiations (a.logits set; craft_tick_policy_stream.hip).
hipError_t launch_tick_stream(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                              hipStream_t st, bool head) {
  if (head) return launch_tick_stream_head(tl, nw, win, tile, v, a, lds, st);
  if (tl == 0) return launch_tile_bare<MODE_STREAM>(win, tile, v, a, lds, st);
  return launch_tile_teach<MODE_STREAM>(tl, nw, win, tile, v, a, lds, st);
}

}  // namespace craft
