// craft_episode_summary.hip — the per-episode results of a queue pass (craft_episode_summary):
// the [ticks][n_envs] records of the four stream entry points cut into results indexed by queue
// entry.  Two launches.  The scan: one lane per slot walks its record column in tick order (a
// wave's loads of one tick are contiguous) and writes each ended episode's length, success,
// pose and actions; a failed get episode's distance it reads from the teacher table, and where
// the table has no answer it leaves a pending marker.  The distance kernel: lane pairs or quads
// per queue entry, all but the pending ones leaving at once, run find_closest_resources' BFS on
// the entry's pool row with nothing cleared, the body of distances_kernel (craft_teacher.hip).
// Neither reads or writes any slot state.
#include "craft_launch.h"
#include "craft_teach.h"

namespace craft {

// distance_out of an entry whose BFS the distance kernel still has to run
constexpr int32_t kDistPending = INT32_MIN;

// Queue entries up to this many run 4 lanes per entry, more run 2 (launch_distances' choice).
constexpr int64_t kSummaryQuadMaxEntries = 16384;

__device__ __forceinline__ bool pose_inside(const SimView& v, int32_t pose) {
  const int x = pose & 0xff, y = (pose >> 8) & 0xff;
  return pose >= 0 && x >= 1 && x <= v.W - 2 && y >= 1 && y <= v.H - 2;
}

// What the scan knows of entry e's distance (craft_rollout_distances' rule for the entry's task,
// this success and this pose): the answer, or kDistPending where only the BFS can tell.
__device__ __forceinline__ int32_t scan_distance(const SimView& v, const SummaryArgs& a, const uint16_t* s_tab,
                                                 int64_t slot, int32_t e, int succ, int32_t pose) {
  const uint2 qe = a.q_entries[e];
  const int task = (int)(qe.x >> 24), scen = (int)(qe.x & 0xffffffu);
  if (task >= v.n_tasks) {
    latch_error(v.err, CRAFT_ERANGE, slot);
    return -2;
  }
  const uint32_t tt = s_tab[task];
  if ((tt & 0xf) != CRAFT_GOAL_GET) return -1;
  if (succ != 0) return 0;
  const int kind = (tt >> 4) & 0xffu;
  int32_t d;
  if (kind == 0) {
    d = -1;                              // kind 0 is never a target (as teach_env)
  } else if (!pose_inside(v, pose) || scen >= v.pool_count) {
    latch_error(v.err, CRAFT_EINVAL, slot);
    d = -2;
  } else {
    const int x = pose & 0xff, y = (pose >> 8) & 0xff, dir = (pose >> 16) & 3;
    const int ts = v.ttab ? tt_slot_of(v, kind) : -1;
    const uint32_t w = ts >= 0 ? tt_row(v, scen * v.tt_nsub)[(ts * 4 + dir) * v.C + x * v.H + y] : 0u;
    if (!(w & 0x8000u)) return kDistPending;
    d = (w & 0x4000u) ? (int32_t)(w & 0x3ffu) - 1 : -2;   // the initial grid is the pool row: the table's answer
  }
  if (d == -1 || d == -2) a.flags[1] = 1;                // len(None), imitation.py:88-89
  return d;
}

// Slot i's recorded actions of rows [start, end) into `row` at positions base, base + 1, ...
// below T: four loads in flight at a time (a slot may end an episode every tick, so the actions
// are read back once the end names the entry; a row is read twice at the most).
__device__ __forceinline__ void copy_actions(int32_t* row, const int32_t* rec, int64_t n, int64_t i, int start,
                                             int end, int base, int T) {
  for (int k = start; k < end && base + (k - start) < T; k += 4) {
    int32_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = rec[(int64_t)min(k + u, end - 1) * n + i];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k + u < end && base + (k + u - start) < T) row[base + (k + u - start)] = v[u];
  }
}

// The scan's records are loaded kScanTicks ticks at a time, every load of the batch in flight
// before the first is used.
constexpr int kScanTicks = 8;

__global__ __launch_bounds__(256) void summary_scan_kernel(SimView v, SummaryArgs a) {
  __shared__ uint16_t s_tab[CRAFT_MAX_TASKS];
  for (int t = threadIdx.x; t < v.n_tasks; t += blockDim.x) s_tab[t] = v.task_tab[t];
  __syncthreads();
  const int64_t n = v.n_envs, i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int T = v.maxT;
  // the running episode: cnt ticks so far; its first tick within the records is row `start`,
  // which is its action number `base` (run[i] until the slot's first end, then 0)
  int base = a.run ? max(a.run[i], 0) : 0;
  int cnt = base, start = 0;
  for (int t0 = 0; t0 < a.ticks; t0 += kScanTicks) {
    int32_t ee[kScanTicks], pp[kScanTicks];
    int8_t ss[kScanTicks];
#pragma unroll
    for (int j = 0; j < kScanTicks; ++j) {
      const int64_t o = (int64_t)min(t0 + j, a.ticks - 1) * n + i;    // (past the last row: its copy, unused)
      ee[j] = a.ep_end[o];
      pp[j] = a.end_pose[o];
      ss[j] = a.success[o];
    }
#pragma unroll
    for (int j = 0; j < kScanTicks; ++j) {
      const int t = t0 + j;
      if (t >= a.ticks) break;
      ++cnt;
      const int32_t e = ee[j];
      if (e < 0) {
        if (e < -1) latch_error(v.err, CRAFT_ERANGE, i);
        continue;
      }
      if ((int64_t)e >= a.q_len) {
        latch_error(v.err, CRAFT_ERANGE, i);
      } else if ((int64_t)e < a.count) {
        const int succ = ss[j];
        a.length_out[e] = cnt;
        a.success_out[e] = (int8_t)succ;
        a.pose_out[e] = pp[j];
        if (succ < 0) a.flags[0] = 1;                      // satisfies() None, imitation.py:68
        if (a.actions_out) {
          int32_t* row = a.actions_out + (int64_t)e * T;
          copy_actions(row, a.rec, n, i, start, t + 1, base, T);
          for (int p = cnt; p < T; ++p) row[p] = -1;
        }
        if (a.dist_out) a.dist_out[e] = scan_distance(v, a, s_tab, i, e, succ, pp[j]);
      }
      cnt = 0;
      base = 0;
      start = t + 1;
    }
  }
  if (a.run) {
    const int32_t now = a.ep_now ? a.ep_now[i] : 0;
    a.run[i] = now < 0 ? 0 : cnt;
    if (a.actions_out && now >= 0 && (int64_t)now < a.count) {   // the running episode's actions so far
      copy_actions(a.actions_out + (int64_t)now * T, a.rec, n, i, start, a.ticks, base, T);
    }
  }
}

// LANES lanes per queue entry; an entry the scan did not leave pending costs one load.  A pending
// one is a failed get episode: success_out is 0 and end_pose_out its final pose, unless a
// CRAFT_QUEUE_WRAP entry ended more than once in the call and another end's stores won, so both
// are read again and the distance written is the one of what they hold.
template <int NW, int LANES>
__global__ __launch_bounds__(256) void summary_distance_kernel(SimView v, SummaryArgs a) {
  __shared__ uint16_t s_tab[CRAFT_MAX_TASKS];
  for (int t = threadIdx.x; t < v.n_tasks; t += blockDim.x) s_tab[t] = v.task_tab[t];
  __syncthreads();
  const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LANES;
  const int ql = (int)(threadIdx.x % LANES);
  if (e >= a.count) return;                              // lane-group-uniform, as every exit below
  if (a.dist_out[e] != kDistPending) return;
  const bool lead = ql == 0;
  const uint2 qe = a.q_entries[e];
  const int task = (int)(qe.x >> 24), scen = (int)(qe.x & 0xffffffu);
  const int32_t pose = a.pose_out[e];
  const int succ = a.success_out[e];
  int d;
  if (succ != 0) {
    d = 0;
  } else if (task >= v.n_tasks || !pose_inside(v, pose) || scen >= v.pool_count) {
    if (lead) latch_error(v.err, CRAFT_EINVAL, e);
    d = -2;
  } else {
    const int C = v.C, H = v.H;
    const int kind = (s_tab[task] >> 4) & 0xffu;
    const int x = pose & 0xff, y = (pose >> 8) & 0xff, dir = (pose >> 16) & 3;
    const Bits<NW> valid = brange<NW>(0, C - 2 * H);     // the band of columns 1 .. W-2
    const uint32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t* row32 = reinterpret_cast<const uint32_t*>(v.pool + (size_t)scen * v.CS);
    Bits<NW> occ, tgt;
    band_bits<NW, LANES>(row32, (C + 3) >> 2, C, H, m, kind, ql, occ, tgt);
    int fa = -1, len = -1;
    const bool ok = bfs_closest<NW, LANES>(occ, tgt, valid, H, x * H + y - H, dir, ql, fa, len, false,
                                           v.pool_conn[scen] != 0);
    // !ok: a target the BFS cannot reach; len -1: no target.  The reference raises the same
    // TypeError for both, so both report through flags[1] and nothing latches
    d = ok ? len : -2;
  }
  if (lead) {
    a.dist_out[e] = d;
    if (d == -1 || d == -2) a.flags[1] = 1;
  }
}

hipError_t launch_episode_summary(int nw, const SimView& v, const SummaryArgs& a, hipStream_t st) {
  if (v.n_envs > 0 && a.ticks > 0) {
    const int64_t blocks = (v.n_envs + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(summary_scan_kernel, dim3((unsigned)blocks), dim3(256), 0, st, v, a);
    if (a.dist_out) {
      const int lanes = a.count <= kSummaryQuadMaxEntries ? 4 : 2;
      const int64_t dblocks = (lanes * a.count + 255) / 256;
      if (dblocks > 0x7fffffffLL) return hipErrorInvalidValue;
      dispatch_nw(nw, [&](auto nwc) {
        constexpr int NW = decltype(nwc)::value;
        if (lanes == 4) hipLaunchKernelGGL((summary_distance_kernel<NW, 4>), dim3((unsigned)dblocks), dim3(256), 0, st, v, a);
        else hipLaunchKernelGGL((summary_distance_kernel<NW, 2>), dim3((unsigned)dblocks), dim3(256), 0, st, v, a);
      });
    }
  }
  return hipGetLastError();
}

}  // namespace craft
