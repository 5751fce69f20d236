// craft_sim.hip — host side of the C ABI (include/craft.h): handle lifetime,
// scenario pool, launches, state I/O and episode statistics.
// Kernels: craft_tile.hip (tick / transition / observe / reset), craft_tick_lang.hip (the
// language trainers' tick), craft_tick_stream.hip (the episode queue and its tick),
// craft_tick_teach.hip (the tick fused with the teacher), craft_rollout_w3/w5/w7.hip (multi-tick),
// craft_rollout_teach.hip (multi-tick with labels), craft_rollout_stream.hip (multi-tick on the
// episode queue), craft_rollout_replay.hip (the same with the actions read from the installed
// tape, and the tape's pack kernel), craft_rollout_teach_stream.hip (both), craft_teacher.hip, craft_scenarios.hip (pool generation).  Their launchers:
// craft_launch.h.
#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "craft_device.h"
#include "craft_checks_episode_summary.h"
#include "craft_checks_lang_policy.h"
#include "craft_checks_lang_stream.h"
#include "craft_checks_policy.h"
#include "craft_checks_rollout_replay.h"
#include "craft_checks_rollout_stream.h"
#include "craft_checks_rollout_teach_stream.h"
#include "craft_host.h"
#include "craft_launch.h"

namespace craft {
namespace {

__global__ void get_state_kernel(SimView v, const int32_t* slots, int64_t n, int32_t* agent_out,
                                 int32_t* inv_out, uint8_t* grid_out, int32_t* spec_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t slot = slots ? (int64_t)slots[i] : i;
  if (slot < 0 || slot >= v.n_envs) { latch_error(v.err, CRAFT_ERANGE, i); return; }
  const Agent s = unpack_state(v.state[slot]);
  if (agent_out) {
    agent_out[4 * i + 0] = s.x;
    agent_out[4 * i + 1] = s.y;
    agent_out[4 * i + 2] = s.dir;
    agent_out[4 * i + 3] = s.timer;
  }
  if (inv_out) {
    const uint8_t* iv = reinterpret_cast<const uint8_t*>(v.inv + 2 * slot);
    for (int k = 0; k < v.K; ++k) inv_out[i * v.K + k] = iv[k];
  }
  if (grid_out) {
    const uint32_t* m = reinterpret_cast<const uint32_t*>(v.mask + 2 * slot);
    const bool ok = s.scen < v.pool_count;
    if ((v.C & 3) == 0) {               // whole dwords: 4 cells per load and per store
      const uint32_t* row = reinterpret_cast<const uint32_t*>(v.pool + (size_t)s.scen * v.CS);
      uint32_t* out = reinterpret_cast<uint32_t*>(grid_out + i * v.C);
      for (int q = 0; q < (v.C >> 2); ++q) {
        uint32_t w = ok ? row[q] : 0u;
        const uint32_t cleared = (m[q >> 3] >> ((q & 7) * 4)) & 0xfu;   // cells 4q..4q+3
        for (int b = 0; b < 4; ++b)
          if ((cleared >> b) & 1u) w &= ~(0xffu << (8 * b));
        out[q] = w;
      }
    } else {
      for (int c = 0; c < v.C; ++c) {
        const int k = ok ? v.pool[(size_t)s.scen * v.CS + c] : 0;
        grid_out[i * v.C + c] = ((m[c >> 5] >> (c & 31)) & 1u) ? 0 : (uint8_t)k;
      }
    }
  }
  if (spec_out) {
    const uint32_t in = v.init[slot];
    spec_out[5 * i + 0] = s.scen;
    spec_out[5 * i + 1] = in & 0xff;
    spec_out[5 * i + 2] = (in >> 8) & 0xff;
    spec_out[5 * i + 3] = (in >> 16) & 3;
    spec_out[5 * i + 4] = s.task;
  }
}

__global__ void set_state_kernel(SimView v, const int32_t* slots, int64_t n, const int32_t* spec_in,
                                 const int32_t* agent_in, const int32_t* inv_in) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t slot = slots ? (int64_t)slots[i] : i;
  if (slot < 0 || slot >= v.n_envs) { latch_error(v.err, CRAFT_ERANGE, i); return; }
  const int sc = spec_in[5 * i], x0 = spec_in[5 * i + 1], y0 = spec_in[5 * i + 2],
            d0 = spec_in[5 * i + 3], tk = spec_in[5 * i + 4];
  const int x = agent_in[4 * i], y = agent_in[4 * i + 1], d = agent_in[4 * i + 2],
            tm = agent_in[4 * i + 3];
  bool ok = sc >= 0 && sc < v.pool_count && tk >= 0 && tk < v.n_tasks && x0 >= 1 &&
            x0 <= v.W - 2 && y0 >= 1 && y0 <= v.H - 2 && d0 >= 0 && d0 < 4 && x >= 1 &&
            x <= v.W - 2 && y >= 1 && y <= v.H - 2 && d >= 0 && d < 4 && tm >= 0 && tm <= 255;
  uint32_t ivw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < v.K; ++k) {
    const int c = inv_in ? inv_in[i * v.K + k] : 0;
    if (c < 0 || c > 255) ok = false;
    ivw[k >> 2] |= (uint32_t)(c & 0xff) << (8 * (k & 3));
  }
  if (!ok) { latch_error(v.err, CRAFT_EINVAL, i); return; }
  Agent s;
  s.x = x; s.y = y; s.dir = d; s.frozen = 0; s.timer = tm; s.scen = sc; s.task = tk;
  v.state[slot] = pack_state(s);
  v.init[slot] = (uint32_t)x0 | ((uint32_t)y0 << 8) | ((uint32_t)d0 << 16);
  v.inv[2 * slot] = make_uint4(ivw[0], ivw[1], ivw[2], ivw[3]);
  v.inv[2 * slot + 1] = make_uint4(ivw[4], ivw[5], ivw[6], ivw[7]);
  v.mask[2 * slot] = make_uint4(0, 0, 0, 0);
  v.mask[2 * slot + 1] = make_uint4(0, 0, 0, 0);
}

__global__ void stats_kernel(int64_t* part, int64_t n_rows, int64_t* out, int reset) {
  __shared__ long long acc[3][256];
  long long s0 = 0, s1 = 0, s2 = 0;
  for (int64_t r = threadIdx.x; r < n_rows; r += blockDim.x) {
    s0 += part[4 * r]; s1 += part[4 * r + 1]; s2 += part[4 * r + 2];
    if (reset) { part[4 * r] = 0; part[4 * r + 1] = 0; part[4 * r + 2] = 0; }
  }
  acc[0][threadIdx.x] = s0; acc[1][threadIdx.x] = s1; acc[2][threadIdx.x] = s2;
  __syncthreads();
  for (int w = blockDim.x / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int j = 0; j < 3; ++j) acc[j][threadIdx.x] += acc[j][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = acc[0][0]; out[1] = acc[1][0]; out[2] = acc[2][0]; }
}

}  // namespace
}  // namespace craft

using craft::SimView;
using craft::TileArgs;

struct craft_sim {
  int device = 0;
  craft_config_t cfg{};
  int64_t n_envs = 0, env_base = 0, n_tiles = 0;
  int32_t pool_capacity = 0, pool_count = 0;
  uint8_t* d_pool = nullptr;
  uint8_t* d_pool_conn = nullptr;   // per pool row: free cells 4-connected (teacher shortcut)
  uint32_t* d_rcw = nullptr;
  uint2* d_wsr = nullptr;           // SimView::wsr: the recipes grouped by workshop, or null
  uint64_t* d_state = nullptr;
  uint32_t* d_init = nullptr;
  uint4* d_inv = nullptr;
  uint4* d_mask = nullptr;
  uint16_t* d_task = nullptr;
  int32_t* d_task_sub = nullptr;
  uint32_t* d_hint = nullptr;       // hint_tables: descriptors + leaf bytes
  int64_t* d_stats = nullptr;
  int32_t* d_err = nullptr;
  uint16_t* d_ttab = nullptr;       // the teacher table (craft_teach.h), or null
  uint8_t* d_ttab4 = nullptr;       // its answers as 4-bit labels (SimView::ttab4)
  uint32_t* d_ttcells = nullptr;    // [pool_capacity][2]: each row's listed clearable cells
  int tt_nslot = 0;                 // target-kind slots of the table
  bool tt_decided = false;          // its size is fixed at the first pool load (ensure_table)
  // pool rows loaded since the table was last built: craft_pool_load only records them, and the
  // next launch that reads the table builds their entries first, on its own stream
  std::vector<std::pair<int32_t, int32_t>> tt_dirty;
  bool hint_walk = false;           // some task keeps the hint walk (no hint table: craft_host.h)
  int32_t tt_kinds[16] = {};        // its slots' target kinds
  SimView view{};
  // The validated knobs (craft_checks.h).  k.teach_table, craft_sim_tune_teach: which teacher reads
  // the table (0 auto: craft_step_teach when the launch rewrites the previous launch's observation
  // buffer, as a trainer's loop does, every other teacher always; 1 always; 2 never).
  craft_host::Knobs k;
  uint8_t* d_sync = nullptr;        // craft_rollout: work-unit counter + per-tile chunk flags
  uint8_t* d_sync_graph = nullptr;  // the same for launches captured into a HIP graph
  size_t sync_bytes = 0;
  bool sync_zeroed = false;         // d_sync zeroed once; then the counter only grows
  int rollout_obs_policy = 2;       // craft_rollout's observation stores until craft_sim_tune sets one:
                                    // write-through, 1.5 % faster than write-back (tools/ab_store.sh)
  bool obs_store_tuned = false;     // craft_sim_tune chose the store policy for every kernel
  uint64_t queue1_next = 0;         // queue[1] (the split kernel's per-unit path) at the next launch
  uint64_t queue_next = 0;          // the counter's value at the next launch (every launch adds
                                    // its units + its grid: one fetch past the end per workgroup)
  // the episode queue (craft_episode_queue / craft_episode_begin / craft_step_stream)
  uint2* d_queue = nullptr;         // packed entries
  int64_t q_count = 0;
  int32_t* d_cursor = nullptr;      // [n_envs] each slot's queue index (-1: run out)
  int32_t* d_qreset = nullptr;      // [5][n_envs] craft_episode_begin's inputs to the reset kernel
  unsigned long long* d_qbad = nullptr;   // the lowest invalid index of a queue being installed
  uint32_t q_step = 0, q_wrap = 0;  // craft_episode_begin's stride (reduced, craft_episode.h) and WRAP
  bool q_begun = false;             // craft_episode_begin since the queue was installed
  uint8_t* d_tape = nullptr;        // craft_episode_actions: [q_count][tape_stride] bytes, or null (no tape)
  int32_t tape_stride = 0;          // max_timesteps rounded up to 4; the rest of a row is STOP
  std::string last_error;
};

namespace {

int fail(craft_sim* sim, int code, const std::string& msg) {
  if (sim) sim->last_error = msg;
  return code;
}

int hip_fail(craft_sim* sim, hipError_t e, const char* what) {
  return fail(sim, CRAFT_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(sim, expr)                                   \
  do {                                                       \
    hipError_t _e = (expr);                                  \
    if (_e != hipSuccess) return hip_fail((sim), _e, #expr); \
  } while (0)

using craft_host::validate_config;

// What the shared argument checks (craft_checks.h) read of the handle.
craft_host::Facts facts(const craft_sim* s) {
  return {&s->cfg, s->n_envs, s->env_base, s->pool_capacity, s->pool_count, s->k.obs_fmt,
          s->d_queue ? s->q_count : 0, s->q_begun};
}

// LDS bytes per tile workgroup (the tile kernel's, craft_tile.h, or with two observation buffers and
// the pristine rows the rollout kernels'); a residency cap R pads the request to 160 KiB / R
// so that at most R tile workgroups share a CU and later tiles' prologues overlap
// earlier tiles' observation stores.
size_t lds_bytes(const craft_sim* s, int tile, int obs_bufs = 1, bool pristine = false) {
  const SimView& v = s->view;
  size_t b = (size_t)craft::lds_layout(tile, v.GS, v.F, obs_bufs, pristine).bytes;
  if (s->k.resident_cap > 0) {
    const size_t capped = ((size_t)163840 / s->k.resident_cap) & ~size_t(15);
    if (capped > b) b = capped;
  }
  return b;
}

// The workgroup shape craft_rollout launches with (craft_sim_rollout_shape).  Default
// (threads 0): for 3x3 windows the split-producer kernel on 32-env tiles with 6
// streaming waves (7-15 % faster than 64-env tiles at 65536 envs);
// otherwise the handle's tile with 256 threads (512 for 64-env tiles).
void rollout_shape(const craft_sim* s, int* tile, int* threads, int* split) {
  // the rollout kernels stage u8 rows (double-buffered): their default tile keeps ~40 KB per buffer
  const int win = s->cfg.window_width;
  int t = s->k.tile_knob ? s->k.tile_knob : (win == 3 ? 64 : (win == 5 ? 32 : 16)), nt = s->k.rollout_threads;
  if (nt == 0 && s->cfg.window_width == 3) {
    t = 32;
    nt = 512;
  }
  // a tile whose two staged observation buffers exceed a workgroup's 160 KiB of LDS (64 envs at
  // 7x7 windows: 300 KB; at 5x5 from 16x16 worlds) cannot launch: it runs as the largest that fits
  while (t > 16 && lds_bytes(s, t, 2, true) > 163840) t /= 2;
  // what launch_rollout_win (craft_rollout.h) instantiates for (t, nt): 64-env tiles run 256
  // or 512 threads, smaller tiles 128, the split kernel at 320 / 384 / 512, else 256
  if (t == 64) nt = (nt == 256) ? 256 : 512;
  else if (nt != 128 && nt != 320 && nt != 384 && nt != 512) nt = 256;
  *tile = t;
  *threads = nt;
  *split = (t <= 32 && nt >= 320) ? 1 : 0;
}

// The one-tile teacher kernel's envs per tile: 64 for 3x3 windows; the handle's tile (default 32)
// for wider ones, whose 64-env observation rows (69 KB at 5x5) leave one workgroup per CU; 32 also
// where 64 envs do not fit a workgroup's LDS (craft_host::tile_fits: 7x7 windows, from 23 kinds on the
// largest worlds).
int teach_tile(const craft_sim* s) {
  const int t = s->cfg.window_width == 3 || s->k.tile != 32 ? craft::kMaxTileEnvs : 32;
  return craft_host::tile_fits(t, s->view.C, s->view.F) ? t : 32;
}

// Teacher lanes per env of the one-tile kernel (craft_sim_tune_teach): quads, or pairs on the
// 32-env tile of wider windows (76.5 against 78.5 us with quads at 5x5), or what the knob says.
int one_tile_lanes(const craft_sim* s) {
  return (s->k.teach_lanes == 1 || s->k.teach_lanes == 2) ? s->k.teach_lanes
         : s->k.teach_lanes == 0 && teach_tile(s) == 32 ? 2 : 4;
}

// What craft_step / craft_step_ex (teach = false) or craft_step_teach (teach = true) launches:
// CRAFT_KERNEL_TILE (craft_tile.h) or CRAFT_KERNEL_TICK2 (craft_tick2.h), with its envs per
// tile / workgroup and teacher lanes per env.
void step_shape(const craft_sim* s, bool teach, int* kernel, int* envs, int* lanes) {
  if (!teach) {
    *kernel = CRAFT_KERNEL_TILE;
    *envs = s->k.tile;
    *lanes = 0;
    return;
  }
  const bool w3 = s->cfg.window_width == 3;
  int k = s->k.teach_kernel;
  // auto: the two-tile kernel for 3x3 windows at the default tile from 32768 envs, where its
  // 128-env workgroups fill the chip, else the one-tile kernel
  if (k == 0) k = (w3 && s->k.tile == craft::kMaxTileEnvs && s->k.resident_cap == 0 && s->n_envs >= 32768) ? 2 : 1;
  if (k == 2 && !(w3 && s->k.tile == craft::kMaxTileEnvs && s->k.resident_cap == 0)) k = 1;
  // teacher lanes per env (craft_sim_tune_teach): the two-tile kernel runs pairs (or quads), the
  // one-tile kernel quads (or pairs, or one lane)
  const int tl2 = s->k.teach_lanes == 4 ? 4 : 2;
  const int tl1 = one_tile_lanes(s);
  if (k == 2) { *kernel = 2; *envs = 128; *lanes = tl2; }
  else { *kernel = 1; *envs = teach_tile(s); *lanes = tl1; }
}

// Builds the teacher-table entries (and listed clearable cells) of the rows loaded since the last
// build, ahead of the launch (`what`) about to read them: on that launch's stream, then a host
// wait, so that a reader on any other stream finds the rows finished too (one wait per batch of
// pool loads, not per launch).  Refused while the stream is being captured into a HIP graph: the
// build would be captured with the launch (rebuilt on every replay, or never run if the capture
// is dropped), so the caller runs one eager launch (or craft_sim_sync_table) first.  Until built,
// a row's entries read as "not computed" (ensure_table's fill), which latches CRAFT_EINVARIANT
// instead of a wrong label.
int flush_table(craft_sim* s, void* stream, const char* what) {
  if (s->tt_dirty.empty()) return CRAFT_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (s->d_ttab) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(s, hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone)
      return fail(s, CRAFT_EINVAL, std::string(what) +
                                       ": pool rows loaded since the last eager teacher launch have no teacher-table "
                                       "entries yet; run craft_sim_sync_table (or one eager launch) before capturing");
    for (const auto& r : s->tt_dirty) {
      const hipError_t e = craft::launch_teach_table(craft::teach_words(s->view.W, s->view.H), s->view, r.first,
                                                     r.second, s->tt_kinds, st);
      if (e != hipSuccess) return hip_fail(s, e, "teacher table build");
    }
    HIP_TRY(s, hipStreamSynchronize(st));
  }
  s->tt_dirty.clear();
  return CRAFT_OK;
}

// The view a teacher launch gets: the table hidden when craft_sim_tune_teach says never.
SimView teach_view(const craft_sim* s) {
  SimView v = s->view;
  if (s->k.teach_table == 2) {
    v.ttab = nullptr;
    v.ttab4 = nullptr;
    v.tt_slots = 0;
  }
  return v;
}

// What one tick of the tile kernel launches with: the view, teacher lanes per env (0: no teacher in
// the launch), words per BFS cell set, envs per tile and LDS bytes.
struct TickPlan {
  SimView v;
  int tl, nw, tile;
  size_t lds;
};

// The plan of `what`'s tick.  Bare: the handle's view and tile, the LDS padded by the residency
// cap.  With the teacher (craft_step_teach's one-tile kernel: its tile, its lanes, its LDS, never
// padded): the table entries of newly loaded rows are built first (flush_table), and the two-tile
// kernel takes the view and nw from here and sizes its own LDS.
int tick_plan(craft_sim* s, bool teach, void* stream, const char* what, TickPlan& p) {
  if (!teach) {
    p = TickPlan{s->view, 0, 0, s->k.tile, lds_bytes(s, s->k.tile)};
    return CRAFT_OK;
  }
  const int rc = flush_table(s, stream, what);
  if (rc != CRAFT_OK) return rc;
  // Teacher-table reads in the fused kernel (its 4-bit copy since round 5): -2.5 us per tick when
  // the launch rewrites the previous launch's observation buffer (a trainer's loop, ring 1), and
  // -0.9 us (30.1 -> 29.2) when every launch writes a fresh slot of a 16-slot ring (round 6,
  // profiles/r06/teach_table_k1; round 4's u16 reads cost +0.5 us there), so auto reads it always.
  p.v = teach_view(s);
  p.v.tt_fused = s->k.teach_table != 2;
  p.tl = one_tile_lanes(s);
  p.nw = craft::teach_words(s->view.W, s->view.H);
  p.tile = teach_tile(s);
  // + task_sub as bytes (the teacher's other words live in row padding and the control words,
  // craft_tile.h): 40,888 bytes for a 32-env tile at 12x12, 5x5, so four workgroups share a CU
  p.lds = (size_t)craft::lds_layout(p.tile, s->view.GS, s->view.F).bytes +
          (((size_t)s->view.n_tasks * CRAFT_MAX_SUBTASKS + 15) & ~size_t(15));
  return CRAFT_OK;
}

int launch(craft_sim* s, int mode, const TileArgs& a, void* stream, const char* what) {
  hipError_t e = craft::launch_tile(mode, s->cfg.window_width, s->k.tile, s->view, a, lds_bytes(s, s->k.tile),
                                    reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(s, e, what);
  return CRAFT_OK;
}

// The sync area of a rollout launch of a.n_ticks ticks on `st`: a.queue, a.tile_done and the
// counters' values at its start (a.qbase, a.qbase1); `captured` says whether it is being captured.
// A launch captured into a HIP graph (torch.cuda.graph) is replayed without this host code, so
// it cannot use the eager launches' running counter: it gets its own sync area, zeroed by a
// memset captured with it, so every replay starts from zero and never touches the eager one.
// The eager area is zeroed once and then its counters only grow: a launch hands out units
// counter - qbase and ends having added what its caller records in queue_next / queue1_next.
// `rezero`: the launch also needs zeroed per-tile flags, so the whole area is zeroed again.
int rollout_sync(craft_sim* s, hipStream_t st, bool rezero, craft::RolloutArgs& a, bool& captured) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_TRY(s, hipStreamIsCapturing(st, &cap));
  captured = cap != hipStreamCaptureStatusNone;
  uint8_t* sync = captured ? s->d_sync_graph : s->d_sync;
  a.queue = reinterpret_cast<unsigned long long*>(sync);
  a.tile_done = reinterpret_cast<uint32_t*>(sync + 16);
  if (a.n_ticks > 0 && (captured || rezero || !s->sync_zeroed)) {
    HIP_TRY(s, hipMemsetAsync(sync, 0, s->sync_bytes, st));
    if (!captured) {
      s->sync_zeroed = true;
      s->queue_next = 0;
      s->queue1_next = 0;
    }
  }
  a.qbase = captured ? 0 : s->queue_next;
  a.qbase1 = captured ? 0 : s->queue1_next;
  return CRAFT_OK;
}

// The cells of a grid that grab, bridge or axe can clear (craft.py:383-410): non-empty cells of a
// grabbable, water or stone kind.
int clearable_cells(const craft_config_t& cfg, const uint8_t* g, int C) {
  int m = 0;
  for (int c = 0; c < C; ++c) {
    const int k = g[c], cls = k < CRAFT_MAX_KINDS ? cfg.kind_class[k] : CRAFT_KIND_INERT;
    m += k != 0 && (cls == CRAFT_KIND_GRABBABLE || cls == CRAFT_KIND_WATER || cls == CRAFT_KIND_STONE);
  }
  return m;
}

// The teacher table's size, fixed at the first pool load from the most clearable cells any row of
// that load has (every grid an env of a row can reach is the row minus a subset of them): tt_m =
// that many (at most 8), fewer while pool_capacity rows x 2^tt_m subsets x slots x 4 directions x C
// cells of u16 exceed 1 GiB or 2^21 table rows (the kernels pack a table row into 21 bits).  12x12
// craft_medium: 6 clearable cells per row, 6 slots: 442 KB per row, 453 MB for 1024 rows.  A row
// with more clearable cells lists its first tt_m; an env that clears another one has no table row
// and its queries run the BFS.  Without room for even the pristine grids (tt_m 0) the table is off.
void ensure_table(craft_sim* s, int max_clearable) {
  if (s->tt_decided) return;
  s->tt_decided = true;
  const int C = s->view.C;
  if (s->tt_nslot == 0) return;
  const size_t budget = (size_t)1 << 30;
  int m = std::min(8, std::max(0, max_clearable));
  const size_t blk = ((size_t)2 * C + 15) & ~(size_t)15;      // SimView::tt_blk
  auto bytes = [&](int mm) { return ((size_t)s->pool_capacity << mm) * s->tt_nslot * 4 * C * sizeof(uint16_t); };
  auto bytes4 = [&](int mm) { return ((size_t)s->pool_capacity << mm) * s->tt_nslot * blk; };
  while (m >= 0 && (bytes(m) + bytes4(m) > budget || ((int64_t)s->pool_capacity << m) >= ((int64_t)1 << 21))) --m;
  if (m < 0) return;
  if (hipMalloc(&s->d_ttab, bytes(m)) != hipSuccess || hipMalloc(&s->d_ttab4, bytes4(m)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(s->d_ttab);
    s->d_ttab = nullptr;                  // no table: every query runs the BFS (same results)
    s->d_ttab4 = nullptr;
    return;
  }
  // every entry "not computed" until its row is built (flush_table): u16 0 and nibble 15 latch
  // CRAFT_EINVARIANT in every reader instead of decoding as a label
  if (hipMemset(s->d_ttab, 0, bytes(m)) != hipSuccess || hipMemset(s->d_ttab4, 0xff, bytes4(m)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(s->d_ttab);
    (void)hipFree(s->d_ttab4);
    s->d_ttab = nullptr;
    s->d_ttab4 = nullptr;
    return;
  }
  s->view.ttab4 = s->d_ttab4;
  s->view.tt_blk = (int32_t)blk;
  s->view.ttab = s->d_ttab;
  s->view.tt_slots = s->tt_nslot;
  s->view.tt_nsub = 1 << m;
}

// The tile kernel's arguments of a (checked) craft_step_args_t.
TileArgs step_args(const craft_sim_t* s, const craft_step_args_t* x) {
  TileArgs a{};
  a.actions = x->actions;
  a.seed = x->action_seed;
  a.tick = x->tick;
  a.flags = x->flags;
  a.n = s->n_envs;
  a.obs = x->obs;
  a.reward = x->reward;
  a.done = x->done;
  a.sat = x->success;
  a.ref = x->ref_actions;
  a.bc = x->behavior_clone;
  a.rec = x->action_record;
  a.any_live = x->any_live;
  a.code = x->transition_code;
  return a;
}

// The same of a (checked) craft_lang_step_args_t.
TileArgs lang_args(const craft_sim_t* s, const craft_lang_step_args_t& x) {
  TileArgs a{};
  a.actions = x.actions;
  a.ref = x.alt_actions;
  a.bc = x.use_alt;
  a.seed = x.action_seed;
  a.tick = x.tick;
  a.n = s->n_envs;
  a.obs = x.obs;
  a.done = x.done;
  a.sat = x.success;
  a.rec = x.action_record;
  a.ask = x.ask_record;
  a.code = x.transition_code;
  a.any_live = x.any_live;
  a.label = x.label_out;
  return a;
}

// Puts the handle's episode queue and a stream entry's three extra outputs on the argument block
// of its kernel (TileArgs or RolloutArgs: the same member names).
template <class ARGS, class X>
void queue_args(const craft_sim_t* s, const X& x, ARGS& a) {
  a.q_entries = s->d_queue;
  a.q_cursor = s->d_cursor;
  a.q_count = (uint32_t)s->q_count;
  a.q_step = s->q_step;
  a.q_wrap = s->q_wrap;
  a.ep_end = x.episode_end;
  a.end_pose = x.end_pose;
  a.ep_now = x.episode_now;
}

// The fields every K-tick launch shares, of a (checked) craft_rollout_stream_args_t or
// craft_rollout_teach_args_t (the same member names).
template <class X>
craft::RolloutArgs rollout_args(const X& x) {
  craft::RolloutArgs a{};
  a.actions = x.actions;
  a.seed = x.action_seed;
  a.tick0 = x.tick0;
  a.n_ticks = x.n_ticks;
  a.ring = x.ring;
  a.flags = x.flags;
  a.obs = x.obs;
  a.reward = x.reward;
  a.done = x.done;
  a.sat = x.success;
  return a;
}

// What the two teacher rollouts add to rollout_args, and the view they launch with.
SimView teach_rollout_args(const craft_sim_t* s, const craft_rollout_teach_args_t& x, craft::RolloutArgs& a) {
  const bool lsync = x.label_actions != 0 || x.behavior_clone != nullptr;
  a.label_in = x.label_in;
  a.bc = x.behavior_clone;
  a.label_actions = x.label_actions != 0;
  // 2: the transition wave looks labels up itself and waits only for BFS answers; 1: it waits
  // for each item's whole row (a task without a hint table: the walk stays with the teacher)
  a.lsync = lsync ? (s->hint_walk ? 1 : 2) : 0;
  a.use_table = s->k.teach_table != 2;              // auto = always: the reads overlap the stream
  a.labels = x.labels;
  a.rec = x.action_record;
  SimView v = teach_view(s);
  // nontemporal observation stores unless tuned: they keep the table's gathered lines in L2
  // (65,536 envs, 20 ticks: 417 -> 388 us with hashed actions, 539 -> 467 us with label actions)
  v.obs_policy = s->obs_store_tuned ? s->rollout_obs_policy : 1;
  return v;
}

// A K-tick launch of one work unit per tile of `tile` envs, all a.n_ticks ticks each
// (craft_rollout_stream, craft_rollout_teach, craft_rollout_teach_stream): the sync area, the
// launch itself (`go(st)`, reading `a`), then the work-unit counter as craft_rollout's split kernel uses it
// (queue[1], one claim past the last unit per workgroup).
template <class GO>
int launch_tile_units(craft_sim_t* s, int tile, craft::RolloutArgs& a, void* stream, const char* what, GO go) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  a.chunk = a.n_ticks;
  bool captured = false;
  const int rc = rollout_sync(s, st, false, a, captured);
  if (rc != CRAFT_OK) return rc;
  int64_t grid = 0;
  a.grid_out = &grid;
  const int64_t units = (s->n_envs + tile - 1) / tile;
  const hipError_t e = go(st);
  if (e != hipSuccess) return hip_fail(s, e, what);
  if (!captured && grid > 0) s->queue1_next += (uint64_t)std::max<int64_t>(units, grid);
  return CRAFT_OK;
}

// The three one-tick launches of (checked) arguments, each shared by an entry point and its
// craft_step_policy* twin: `head` null = the actions are given or hashed, else the policy head's
// (the same launchers and tick plan, the kernels' head instantiations).
void head_args(const craft_policy_head_t* head, TileArgs& a) {
  if (!head) return;
  a.logits = head->logits;
  a.head_mode = head->mode;
  a.head_seed = head->seed;
}

int run_step(craft_sim_t* s, const craft_step_args_t* x, const craft_policy_head_t* head, void* stream) {
  TileArgs a = step_args(s, x);
  head_args(head, a);
  return launch(s, head ? craft::MODE_TICK_HEAD : craft::MODE_TICK, a, stream, "craft_step launch");
}

int run_step_teach(craft_sim_t* s, const craft_step_args_t* x, const craft_policy_head_t* head, int32_t* label_out,
                   void* stream, const char* what) {
  TileArgs a = step_args(s, x);
  a.label = label_out;
  head_args(head, a);
  int kernel = 0, envs = 0, tl = 0;
  step_shape(s, true, &kernel, &envs, &tl);
  TickPlan p;
  const int rc = tick_plan(s, true, stream, what, p);
  if (rc != CRAFT_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const hipError_t e =
      kernel == 2 ? craft::launch_tick2(tl, p.nw, p.v, a, craft::tick2_lds_bytes(tl, p.nw, s->view.GS, s->view.F), st,
                                        head != nullptr)
                  : craft::launch_tick_teach(p.tl, p.nw, s->cfg.window_width, p.tile, p.v, a, p.lds, st, head != nullptr);
  if (e != hipSuccess) return hip_fail(s, e, (std::string(what) + " launch").c_str());
  return CRAFT_OK;
}

int run_step_stream(craft_sim_t* s, const craft_stream_step_args_t* x, const craft_policy_head_t* head, void* stream,
                    const char* what) {
  TileArgs a = step_args(s, &x->step);
  a.label = x->label_out;
  queue_args(s, *x, a);
  head_args(head, a);
  TickPlan p;
  const int rc = tick_plan(s, x->label_out != nullptr, stream, what, p);
  if (rc != CRAFT_OK) return rc;
  const hipError_t e = craft::launch_tick_stream(p.tl, p.nw, s->cfg.window_width, p.tile, p.v, a, p.lds,
                                                 reinterpret_cast<hipStream_t>(stream), head != nullptr);
  if (e != hipSuccess) return hip_fail(s, e, (std::string(what) + " launch").c_str());
  return CRAFT_OK;
}

// The language ticks likewise, each shared with its craft_step_lang_policy* twin: `head` the
// main row's head, `alt` the alt row's (null: alt_actions are integers, or there are none).
void lang_head_args(const craft_policy_head_t* head, const craft_policy_head_t* alt, TileArgs& a) {
  head_args(head, a);
  if (!alt) return;
  a.alt_logits = alt->logits;
  a.alt_mode = alt->mode;
  a.alt_seed = alt->seed;
}

int run_step_lang(craft_sim_t* s, const craft_lang_step_args_t* x, const craft_policy_head_t* head,
                  const craft_policy_head_t* alt, void* stream, const char* what) {
  TileArgs a = lang_args(s, *x);
  lang_head_args(head, alt, a);
  TickPlan p;
  const int rc = tick_plan(s, x->label_out != nullptr, stream, what, p);
  if (rc != CRAFT_OK) return rc;
  const hipError_t e = craft::launch_tick_lang(p.tl, p.nw, s->cfg.window_width, p.tile, p.v, a, p.lds,
                                               reinterpret_cast<hipStream_t>(stream), head != nullptr);
  if (e != hipSuccess) return hip_fail(s, e, (std::string(what) + " launch").c_str());
  return CRAFT_OK;
}

int run_step_lang_stream(craft_sim_t* s, const craft_lang_stream_step_args_t* x, const craft_policy_head_t* head,
                         const craft_policy_head_t* alt, void* stream, const char* what) {
  TileArgs a = lang_args(s, x->step);
  queue_args(s, *x, a);
  lang_head_args(head, alt, a);
  TickPlan p;
  const int rc = tick_plan(s, x->step.label_out != nullptr, stream, what, p);
  if (rc != CRAFT_OK) return rc;
  const hipError_t e = craft::launch_tick_lang_stream(p.tl, p.nw, s->cfg.window_width, p.tile, p.v, a, p.lds,
                                                      reinterpret_cast<hipStream_t>(stream), head != nullptr);
  if (e != hipSuccess) return hip_fail(s, e, (std::string(what) + " launch").c_str());
  return CRAFT_OK;
}

}  // namespace

extern "C" {

const char* craft_strerror(int status) { return craft_host::status_text(status); }

int craft_host_flag_pointer(void* host, int32_t** device_out) {
  if (!host || !device_out) return CRAFT_EINVAL;
  *device_out = nullptr;
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess || !d) {
    (void)hipGetLastError();
    return CRAFT_EINVAL;                    // not page-locked host memory HIP knows
  }
  *device_out = static_cast<int32_t*>(d);
  return CRAFT_OK;
}

int craft_sim_create(const craft_config_t* cfg, int device, int64_t n_envs, int64_t env_id_base,
                     int32_t pool_capacity, craft_sim_t** out) {
  if (!cfg || !out || n_envs <= 0 || pool_capacity <= 0 || pool_capacity > (1 << 24) || env_id_base < 0)
    return CRAFT_EINVAL;
  *out = nullptr;
  std::string msg;
  int rc = validate_config(cfg, msg);
  if (rc) {
    fprintf(stderr, "craft_sim_create: %s\n", msg.c_str());
    return rc;
  }
  craft_sim* s = new craft_sim();
  s->device = device;
  s->cfg = *cfg;
  s->n_envs = n_envs;
  s->env_base = env_id_base;
  s->pool_capacity = pool_capacity;
  // stats rows: one per 16-env tile, plus the step kernel's last workgroup's tick waves (its
  // wave count is rounded up to the workgroup's 4)
  s->n_tiles = (n_envs + craft::kMinTileEnvs - 1) / craft::kMinTileEnvs + 4;
  s->k.tile = craft_host::default_tile(cfg->window_width);
  const int W = cfg->width, H = cfg->height, K = cfg->n_kinds, F = cfg->n_features;
  const int C = W * H, CS = (C + 15) & ~15;
  const int GS = CS + 4;                  // odd dword stride: lane-private rows hit distinct banks
  uint32_t rcw[CRAFT_MAX_RECIPES * 3] = {};          // SimView::rcw packing (craft_device.h)
  for (int r = 0; r < cfg->n_recipes; ++r) {
    const craft_recipe_t& rc = cfg->recipe[r];
    uint8_t b[12] = {};
    b[0] = (uint8_t)rc.output;
    b[1] = (uint8_t)rc.workshop;
    b[2] = (uint8_t)rc.n_inputs;
    for (int i = 0; i < rc.n_inputs; ++i) {
      b[3 + 2 * i] = (uint8_t)rc.input_kind[i];
      b[4 + 2 * i] = (uint8_t)rc.input_count[i];
    }
    b[11] = (uint8_t)rc.yield;                       // 1..255 (validated)
    for (int q = 0; q < 3; ++q)
      rcw[3 * r + q] = (uint32_t)b[4 * q] | ((uint32_t)b[4 * q + 1] << 8) | ((uint32_t)b[4 * q + 2] << 16) |
                       ((uint32_t)b[4 * q + 3] << 24);
  }
  // SimView::wsr: workshop k's recipes in dict order, compact, kWsSlots slots per kind (the
  // fourth of each kind's 4 stays zero)
  std::vector<uint2> wsr((size_t)CRAFT_MAX_KINDS * 4, make_uint2(0, 0));
  bool wsr_ok = true;
  {
    int used[CRAFT_MAX_KINDS] = {};
    for (int r = 0; r < cfg->n_recipes; ++r) {
      const craft_recipe_t& rc = cfg->recipe[r];
      const int k = rc.workshop;
      if (k <= 0 || k >= CRAFT_MAX_KINDS || used[k] >= craft::kWsSlots || rc.n_inputs > 2) {
        wsr_ok = false;
        continue;
      }
      const uint32_t k0 = rc.n_inputs > 0 ? (uint32_t)rc.input_kind[0] : 0u, c0 = rc.n_inputs > 0 ? (uint32_t)rc.input_count[0] : 0u;
      const uint32_t k1 = rc.n_inputs > 1 ? (uint32_t)rc.input_kind[1] : 0u, c1 = rc.n_inputs > 1 ? (uint32_t)rc.input_count[1] : 0u;
      wsr[(size_t)k * 4 + used[k]++] = make_uint2((uint32_t)rc.output | ((uint32_t)k << 8) | (k0 << 16) | (k1 << 24),
                                                  c0 | (c1 << 8) | ((uint32_t)rc.yield << 16));
    }
  }
  std::vector<uint16_t> task_tab(CRAFT_MAX_TASKS, 0);
  std::vector<int32_t> task_sub(CRAFT_MAX_TASKS * CRAFT_MAX_SUBTASKS, 0);
  craft_host::task_tables(*cfg, task_tab.data(), task_sub.data());
  std::vector<uint32_t> hint(CRAFT_MAX_TASKS * 4, 0);
  std::vector<uint8_t> hint_leaf;
  craft_host::hint_tables(*cfg, task_tab.data(), task_sub.data(), hint.data(), hint_leaf);
  const size_t hint_bytes = hint.size() * 4 + ((hint_leaf.size() + 15) & ~size_t(15));
  hint.resize(hint_bytes / 4, 0u);
  if (!hint_leaf.empty()) memcpy(hint.data() + CRAFT_MAX_TASKS * 4, hint_leaf.data(), hint_leaf.size());
  auto cleanup = [&](hipError_t e, const char* what) {
    fprintf(stderr, "craft_sim_create: %s: %s\n", what, hipGetErrorString(e));
    craft_sim_destroy(s);
    return CRAFT_EHIP;
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return cleanup(e, "hipSetDevice");
#define ALLOC(ptr, bytes)                                                          \
  do {                                                                             \
    if ((e = hipMalloc(&(ptr), (bytes))) != hipSuccess) return cleanup(e, #ptr);   \
    if ((e = hipMemset((ptr), 0, (bytes))) != hipSuccess) return cleanup(e, #ptr); \
  } while (0)
  ALLOC(s->d_pool, (size_t)pool_capacity * CS);
  ALLOC(s->d_pool_conn, (size_t)pool_capacity + 16);
  ALLOC(s->d_state, sizeof(uint64_t) * n_envs);
  ALLOC(s->d_init, sizeof(uint32_t) * n_envs);
  ALLOC(s->d_inv, 2 * sizeof(uint4) * n_envs);
  ALLOC(s->d_mask, 2 * sizeof(uint4) * n_envs);
  ALLOC(s->d_task, sizeof(uint16_t) * task_tab.size());
  ALLOC(s->d_rcw, sizeof(rcw));
  if (wsr_ok) ALLOC(s->d_wsr, sizeof(uint2) * wsr.size());
  ALLOC(s->d_task_sub, sizeof(int32_t) * task_sub.size());
  ALLOC(s->d_hint, hint_bytes);
  ALLOC(s->d_stats, 4 * sizeof(int64_t) * s->n_tiles);
  ALLOC(s->d_err, 4 * sizeof(int32_t));
  s->sync_bytes = (16 + 4 * (size_t)((n_envs + 15) / 16) + 15) & ~size_t(15);   // queue + tile_done
  ALLOC(s->d_sync, s->sync_bytes);
  ALLOC(s->d_sync_graph, s->sync_bytes);      // craft_rollout launches captured into a graph
  // The teacher table: one slot per kind some go[] or get[] task targets (teach_env's BFS kinds
  // and the rollout summary's); its size is fixed at the first pool load (ensure_table).
  // craft_sim_tune_teach(.., table 2) stops every teacher reading it (the parity switch).
  ALLOC(s->d_ttcells, (size_t)pool_capacity * 2 * sizeof(uint32_t));
  {
    int nslot = 0;
    uint64_t smap[2] = {~0ull, ~0ull};
    for (int t = 0; t < cfg->n_tasks; ++t) {
      const craft_task_t& tk = cfg->task[t];
      const int k = tk.arg_kind;
      if ((tk.goal != CRAFT_GOAL_GO && tk.goal != CRAFT_GOAL_GET) || k <= 0 || k >= 32) continue;
      if (((smap[k >> 4] >> (4 * (k & 15))) & 0xfull) != 0xfull) continue;      // has a slot
      if (nslot >= 15) continue;                                                    // no room: BFS
      smap[k >> 4] &= ~(0xfull << (4 * (k & 15)));
      smap[k >> 4] |= (uint64_t)nslot << (4 * (k & 15));
      s->tt_kinds[nslot++] = k;
    }
    s->tt_nslot = nslot;
    s->view.tt_slot[0] = smap[0];
    s->view.tt_slot[1] = smap[1];
  }
#undef ALLOC
  if ((e = hipMemcpy(s->d_task, task_tab.data(), sizeof(uint16_t) * task_tab.size(), hipMemcpyHostToDevice)) != hipSuccess)
    return cleanup(e, "task table");
  if ((e = hipMemcpy(s->d_rcw, rcw, sizeof(rcw), hipMemcpyHostToDevice)) != hipSuccess)
    return cleanup(e, "recipe table");
  if (s->d_wsr && (e = hipMemcpy(s->d_wsr, wsr.data(), sizeof(uint2) * wsr.size(), hipMemcpyHostToDevice)) != hipSuccess)
    return cleanup(e, "workshop recipe table");
  if ((e = hipMemcpy(s->d_task_sub, task_sub.data(), sizeof(int32_t) * task_sub.size(), hipMemcpyHostToDevice)) != hipSuccess)
    return cleanup(e, "subtask table");
  if ((e = hipMemcpy(s->d_hint, hint.data(), hint_bytes, hipMemcpyHostToDevice)) != hipSuccess)
    return cleanup(e, "hint table");

  SimView& v = s->view;
  v.pool = s->d_pool;
  v.pool_conn = s->d_pool_conn;
  v.state = s->d_state;
  v.init = s->d_init;
  v.inv = s->d_inv;
  v.mask = s->d_mask;
  v.task_tab = s->d_task;
  v.task_sub = s->d_task_sub;
  v.hint = s->d_hint;
  v.hint_bytes = (int32_t)hint_leaf.size();
  for (int t = 0; t < cfg->n_tasks; ++t) s->hint_walk |= (hint[4 * t + 2] & craft_host::kHintWalk) != 0;
  v.stats_part = s->d_stats;
  v.err = s->d_err;
  v.ttab = nullptr;                       // (until the first pool load: ensure_table)
  v.ttab4 = nullptr;
  v.tt_blk = 0;
  v.tt_cells = s->d_ttcells;
  v.tt_nsub = 1;
  v.n_envs = n_envs;
  v.env_base = env_id_base;
  v.pool_count = 0;
  v.n_tasks = cfg->n_tasks;
  v.n_recipes = cfg->n_recipes;
  v.W = W; v.H = H; v.K = K; v.F = F; v.C = C; v.CS = CS; v.GS = GS;
  v.maxT = cfg->max_timesteps;
  v.bridge = cfg->bridge_kind;
  // write-through (sc1) observation stores: with one observation buffer rewritten every tick (a
  // trainer's, do_rollout's) the tick kernel takes 20.3 us against 26.4 with nontemporal stores,
  // and 27.0 against 26.5 when every tick writes a fresh slot of a 1.7 GB ring (tools/step_probe.py)
  v.obs_policy = 2;
  v.obs_fmt = CRAFT_OBS_F32;
  v.axe = cfg->axe_kind;
  v.kc_lo = v.kc_hi = 0;
  for (int k = 0; k < CRAFT_MAX_KINDS; ++k) {
    const uint64_t cls = cfg->kind_class[k] & 0xf;
    if (k < 16) v.kc_lo |= cls << (4 * k);
    else v.kc_hi |= cls << (4 * (k - 16));
  }
  v.rcw = s->d_rcw;
  v.wsr = s->d_wsr;
  *out = s;
  return CRAFT_OK;
}

int craft_sim_tune(craft_sim_t* s, int32_t tile_envs, int32_t max_resident_per_cu, int32_t obs_store) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::set_tune(s->k, s->cfg.window_width, s->view.C, s->view.F, tile_envs,
                                          max_resident_per_cu, obs_store, s->last_error))
    return rc;
  s->view.obs_policy = obs_store;
  s->rollout_obs_policy = obs_store;
  s->obs_store_tuned = true;
  return CRAFT_OK;
}

int craft_sim_tune_teach(craft_sim_t* s, int32_t kernel, int32_t lanes, int32_t table) {
  if (!s) return CRAFT_EINVAL;
  return craft_host::set_tune_teach(s->k, kernel, lanes, table, s->last_error);
}

// Test hook, not part of include/craft.h (host code only, no device needed): craft_host::tile_fits
// restates the size of the one-tick carve by hand, so that both libraries can refuse a tile;
// this counts the (tile, WIDTH*HEIGHT, window, kinds) of the ABI's ranges for which it says "fits"
// while lds_layout plus the teacher tick's subtask bytes (tick_plan) exceed a workgroup's LDS, or
// for which the carve is larger than the bound tile_fits compares.  Both counts must stay 0
// (tests/test_cookbook_limits.py); *checked = the combinations looked at.
int craft_debug_tile_fits_drift(int64_t* checked) {
  int bad = 0;
  int64_t n = 0;
  const size_t sub = ((size_t)CRAFT_MAX_TASKS * CRAFT_MAX_SUBTASKS + 15) & ~size_t(15);
  for (int tile = craft::kMinTileEnvs; tile <= craft::kMaxTileEnvs; tile *= 2)
    for (int cells = 9; cells <= CRAFT_MAX_CELLS; ++cells)
      for (int win = 3; win <= 7; win += 2)
        for (int K = 2; K <= CRAFT_MAX_KINDS; ++K, ++n) {
          const int F = 2 * win * win * K + K + 5, GS = ((cells + 15) & ~15) + 4;
          const size_t carve = (size_t)craft::lds_layout(tile, GS, F).bytes + sub;
          if ((int64_t)carve > craft_host::tile_lds_bound(tile, cells, F) ||
              (craft_host::tile_fits(tile, cells, F) && carve > 163840))
            ++bad;
        }
  if (checked) *checked = n;
  return bad;
}

int craft_abi_version(void) { return CRAFT_ABI_VERSION; }

int craft_sim_tune_host(craft_sim_t* s, int32_t threads) {
  if (!s) return CRAFT_EINVAL;
  return craft_host::check_tune_host(threads, s->last_error);   // (no host workers in this library)
}

int craft_sim_sync_table(craft_sim_t* s, void* stream) {
  if (!s) return CRAFT_EINVAL;
  HIP_TRY(s, hipSetDevice(s->device));
  return flush_table(s, stream, "craft_sim_sync_table");
}

int craft_sim_step_shape(const craft_sim_t* s, int32_t teach, int32_t* kernel, int32_t* envs, int32_t* lanes) {
  if (!s) return CRAFT_EINVAL;
  int k = 0, e = 0, l = 0;
  step_shape(s, teach != 0, &k, &e, &l);
  if (kernel) *kernel = k;
  if (envs) *envs = e;
  if (lanes) *lanes = l;
  return CRAFT_OK;
}

int craft_sim_tune_rollout(craft_sim_t* s, int32_t chunk_ticks, int32_t threads) {
  if (!s) return CRAFT_EINVAL;
  return craft_host::set_tune_rollout(s->k, chunk_ticks, threads, s->last_error);
}

int craft_sim_set_obs_format(craft_sim_t* s, int32_t format) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::set_obs_format(s->k, format, s->last_error)) return rc;
  s->view.obs_fmt = format;
  return CRAFT_OK;
}

int craft_sim_destroy(craft_sim_t* s) {
  if (!s) return CRAFT_OK;
  (void)hipSetDevice(s->device);
  (void)hipFree(s->d_pool);
  (void)hipFree(s->d_pool_conn);
  (void)hipFree(s->d_state);
  (void)hipFree(s->d_init);
  (void)hipFree(s->d_inv);
  (void)hipFree(s->d_mask);
  (void)hipFree(s->d_task);
  (void)hipFree(s->d_rcw);
  (void)hipFree(s->d_wsr);
  (void)hipFree(s->d_task_sub);
  (void)hipFree(s->d_hint);
  (void)hipFree(s->d_stats);
  (void)hipFree(s->d_err);
  (void)hipFree(s->d_sync);
  (void)hipFree(s->d_sync_graph);
  (void)hipFree(s->d_ttab);
  (void)hipFree(s->d_ttab4);
  (void)hipFree(s->d_ttcells);
  (void)hipFree(s->d_queue);
  (void)hipFree(s->d_tape);
  (void)hipFree(s->d_cursor);
  (void)hipFree(s->d_qreset);
  (void)hipFree(s->d_qbad);
  delete s;
  return CRAFT_OK;
}

const char* craft_sim_last_error(const craft_sim_t* s) { return s ? s->last_error.c_str() : "null handle"; }

int craft_sim_info(const craft_sim_t* s, int64_t* n_envs, int32_t* pool_capacity, int32_t* n_features) {
  if (!s) return CRAFT_EINVAL;
  if (n_envs) *n_envs = s->n_envs;
  if (pool_capacity) *pool_capacity = s->pool_capacity;
  if (n_features) *n_features = s->cfg.n_features;
  return CRAFT_OK;
}

int craft_sim_rollout_shape(const craft_sim_t* s, int32_t* tile_envs, int32_t* threads, int32_t* split) {
  if (!s) return CRAFT_EINVAL;
  int t = 0, nt = 0, sp = 0;
  rollout_shape(s, &t, &nt, &sp);
  if (tile_envs) *tile_envs = t;
  if (threads) *threads = nt;
  if (split) *split = sp;
  return CRAFT_OK;
}

int craft_sim_tile_shape(const craft_sim_t* s, int32_t* tile_envs, int32_t* obs_store) {
  if (!s) return CRAFT_EINVAL;
  if (tile_envs) *tile_envs = s->k.tile;
  if (obs_store) *obs_store = s->view.obs_policy;
  return CRAFT_OK;
}

int craft_sim_check(craft_sim_t* s, int64_t* env_out, void* stream) {
  if (!s) return CRAFT_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int32_t h[4] = {0, 0, 0, 0};
  HIP_TRY(s, hipMemcpyAsync(h, s->d_err, sizeof(h), hipMemcpyDeviceToHost, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  if (h[0]) {
    HIP_TRY(s, hipMemsetAsync(s->d_err, 0, sizeof(h), st));
    HIP_TRY(s, hipStreamSynchronize(st));
    const int64_t slot = (int64_t)(uint32_t)h[2] | ((int64_t)h[3] << 32);
    if (env_out) *env_out = slot;
    return fail(s, h[0], std::string(craft_strerror(h[0])) + " (slot/item " + std::to_string(slot) + ")");
  }
  if (env_out) *env_out = -1;
  return CRAFT_OK;
}

int craft_sim_error_word(craft_sim_t* s, int32_t* out, void* stream) {
  if (!s || !out) return CRAFT_EINVAL;
  HIP_TRY(s, hipMemcpyAsync(out, s->d_err, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice,
                            reinterpret_cast<hipStream_t>(stream)));
  return CRAFT_OK;
}

int craft_pool_load(craft_sim_t* s, const uint8_t* grids, int32_t first, int32_t count) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_pool_load(facts(s), grids, first, count, s->last_error)) return rc;
  const int C = s->cfg.width * s->cfg.height, CS = s->view.CS;
  std::vector<uint8_t> staged((size_t)count * CS, 0);
  std::vector<uint8_t> conn((size_t)count, 0);
  for (int p = 0; p < count; ++p) {
    const uint8_t* g = grids + (size_t)p * C;
    std::string msg;
    const int rc = craft_host::check_pool_grid(s->cfg, g, (int64_t)first + p, msg, &conn[p]);
    if (rc) return fail(s, rc, msg);
    std::memcpy(staged.data() + (size_t)p * CS, g, C);
  }
  HIP_TRY(s, hipSetDevice(s->device));
  if (count) {
    int maxm = 0;
    for (int p = 0; p < count; ++p) maxm = std::max(maxm, clearable_cells(s->cfg, grids + (size_t)p * C, C));
    ensure_table(s, maxm);
    HIP_TRY(s, hipMemcpy(s->d_pool + (size_t)first * CS, staged.data(), staged.size(), hipMemcpyHostToDevice));
    HIP_TRY(s, hipMemcpy(s->d_pool_conn + first, conn.data(), count, hipMemcpyHostToDevice));
    // the rows' teacher-table entries: built by the next launch that reads the table (flush_table)
    if (!s->tt_dirty.empty() && s->tt_dirty.back().first + s->tt_dirty.back().second == first)
      s->tt_dirty.back().second += count;
    else
      s->tt_dirty.emplace_back(first, count);
  }
  if (first + count > s->pool_count) s->pool_count = first + count;
  s->view.pool_count = s->pool_count;
  return CRAFT_OK;
}

int craft_pool_generate(craft_sim_t* s, uint64_t seed, int64_t scenario_id0, int32_t first, int32_t count,
                        int32_t boundary_kind, const int32_t* primitives, int32_t n_primitive_kinds,
                        int32_t n_per_primitive, const int32_t* workshop_kind, int32_t n_workshops,
                        int32_t* init_pos_out, void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_pool_generate(facts(s), first, count, boundary_kind, primitives,
                                                     n_primitive_kinds, n_per_primitive, workshop_kind, n_workshops,
                                                     s->last_error))
    return rc;
  craft::ScenarioArgs a{};
  a.seed = seed;
  a.id0 = scenario_id0;
  a.count = count;
  a.first = first;
  a.boundary = boundary_kind;
  a.n_prim = n_primitive_kinds;
  a.n_per = n_per_primitive;
  a.n_ws = n_workshops;
  for (int i = 0; i < n_primitive_kinds; ++i) a.prim[i] = primitives[i];
  for (int i = 0; i < n_workshops; ++i) a.ws[i] = workshop_kind[i];
  a.init_out = init_pos_out;
  HIP_TRY(s, hipSetDevice(s->device));
  {
    // the generated rows' clearable cells: n_per_primitive of each clearable primitive kind, and
    // the clearable workshop kinds
    auto clearable = [&](int k) {
      const int cls = s->cfg.kind_class[k];
      return cls == CRAFT_KIND_GRABBABLE || cls == CRAFT_KIND_WATER || cls == CRAFT_KIND_STONE;
    };
    int maxm = 0;
    for (int i = 0; i < n_primitive_kinds; ++i) maxm += clearable(primitives[i]) ? n_per_primitive : 0;
    for (int i = 0; i < n_workshops; ++i) maxm += clearable(workshop_kind[i]) ? 1 : 0;
    if (count) ensure_table(s, maxm);
  }
  hipError_t e = craft::launch_scenarios(s->view, a, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(s, e, "craft_pool_generate launch");
  e = craft::launch_teach_table(craft::teach_words(s->view.W, s->view.H), s->view, first, count, s->tt_kinds,
                                reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(s, e, "craft_pool_generate teacher table");
  if (first + count > s->pool_count) s->pool_count = first + count;
  s->view.pool_count = s->pool_count;
  return CRAFT_OK;
}

int craft_reset(craft_sim_t* s, const int32_t* scenario, const int32_t* pos_x, const int32_t* pos_y,
                const int32_t* dir, const int32_t* task, void* obs, void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_reset(scenario, pos_x, pos_y, dir, task, obs, s->last_error)) return rc;
  TileArgs a{};
  a.r_scen = scenario; a.r_x = pos_x; a.r_y = pos_y; a.r_dir = dir; a.r_task = task;
  a.n = s->n_envs;
  a.obs = obs;
  int rc = launch(s, craft::MODE_RESET, a, stream, "craft_reset launch");
  if (rc) return rc;
  HIP_TRY(s, hipMemsetAsync(s->d_stats, 0, 4 * sizeof(int64_t) * s->n_tiles, reinterpret_cast<hipStream_t>(stream)));
  return CRAFT_OK;
}

int craft_step(craft_sim_t* s, const int32_t* actions, uint64_t action_seed, int64_t tick, uint32_t flags,
               void* obs, float* reward, uint8_t* done, int8_t* success, void* stream) {
  craft_step_args_t x{};
  x.actions = actions;
  x.action_seed = action_seed;
  x.tick = tick;
  x.flags = flags;
  x.obs = obs;
  x.reward = reward;
  x.done = done;
  x.success = success;
  return craft_step_ex(s, &x, stream);
}

int craft_step_teach(craft_sim_t* s, const craft_step_args_t* x, int32_t* label_out, void* stream) {
  if (!s || !x || !label_out) return CRAFT_EINVAL;
  int rc = craft_host::check_step_teach(facts(s), x, s->last_error);
  if (rc != CRAFT_OK) return rc;
  return run_step_teach(s, x, nullptr, label_out, stream, "craft_step_teach");
}

int craft_policy_actions(craft_sim_t* s, const craft_policy_head_t* head, int64_t tick, int32_t* actions_out,
                         void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_policy_actions(head, actions_out, s->last_error)) return rc;
  const hipError_t e = craft::launch_policy_actions(head->logits, head->mode, head->seed, s->env_base, tick, s->n_envs,
                                                    actions_out, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(s, e, "craft_policy_actions launch");
  return CRAFT_OK;
}

int craft_step_policy(craft_sim_t* s, const craft_step_args_t* x, const craft_policy_head_t* head, int32_t* label_out,
                      void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_step_policy(facts(s), x, head, label_out, s->last_error)) return rc;
  return label_out ? run_step_teach(s, x, head, label_out, stream, "craft_step_policy") : run_step(s, x, head, stream);
}

int craft_step_policy_stream(craft_sim_t* s, const craft_stream_step_args_t* x, const craft_policy_head_t* head,
                             void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_step_policy_stream(facts(s), x, head, s->last_error)) return rc;
  return run_step_stream(s, x, head, stream, "craft_step_policy_stream");
}

int craft_step_lang(craft_sim_t* s, const craft_lang_step_args_t* x, void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_step_lang(facts(s), x, s->last_error)) return rc;
  return run_step_lang(s, x, nullptr, nullptr, stream, "craft_step_lang");
}

int craft_policy_ask(craft_sim_t* s, const craft_policy_head_t* head, float threshold, uint8_t* ask_out,
                     void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_policy_ask(head, threshold, ask_out, s->last_error)) return rc;
  const hipError_t e =
      craft::launch_policy_ask(head->logits, threshold, s->n_envs, ask_out, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(s, e, "craft_policy_ask launch");
  return CRAFT_OK;
}

int craft_step_lang_policy(craft_sim_t* s, const craft_lang_step_args_t* x, const craft_policy_head_t* head,
                           const craft_policy_head_t* alt_head, void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_step_lang_policy(facts(s), x, head, alt_head, s->last_error)) return rc;
  return run_step_lang(s, x, head, alt_head, stream, "craft_step_lang_policy");
}

int craft_step_lang_policy_stream(craft_sim_t* s, const craft_lang_stream_step_args_t* x,
                                  const craft_policy_head_t* head, const craft_policy_head_t* alt_head,
                                  void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_step_lang_policy_stream(facts(s), x, head, alt_head, s->last_error)) return rc;
  return run_step_lang_stream(s, x, head, alt_head, stream, "craft_step_lang_policy_stream");
}

int craft_episode_queue(craft_sim_t* s, const int32_t* specs, int64_t count) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_episode_queue(specs, count, s->last_error)) return rc;
  HIP_TRY(s, hipSetDevice(s->device));
  // the handle's own buffers, once: the cursors, craft_episode_begin's reset inputs, the check's word
  if (!s->d_cursor) {
    int32_t* cur = nullptr;
    int32_t* rs = nullptr;
    unsigned long long* bad = nullptr;
    const size_t nb = (size_t)std::max<int64_t>(s->n_envs, 1) * sizeof(int32_t);
    if (hipMalloc(&cur, nb) != hipSuccess || hipMalloc(&rs, 5 * nb) != hipSuccess ||
        hipMalloc(&bad, sizeof(unsigned long long)) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(cur);
      (void)hipFree(rs);
      (void)hipFree(bad);
      return fail(s, CRAFT_ENOMEM, "craft_episode_queue: out of device memory");
    }
    s->d_cursor = cur;
    s->d_qreset = rs;
    s->d_qbad = bad;
  }
  uint2* q = nullptr;
  if (hipMalloc(&q, (size_t)count * sizeof(uint2)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(s, CRAFT_ENOMEM, "craft_episode_queue: out of device memory");
  }
  unsigned long long bad = ~0ull;
  hipError_t e = hipMemcpy(s->d_qbad, &bad, sizeof(bad), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = craft::launch_queue_pack(s->view, specs, count, q, s->d_qbad, nullptr);
  if (e == hipSuccess) e = hipMemcpy(&bad, s->d_qbad, sizeof(bad), hipMemcpyDeviceToHost);   // (waits for the kernel)
  if (e != hipSuccess) {
    (void)hipFree(q);
    return hip_fail(s, e, "craft_episode_queue");
  }
  if (bad != ~0ull) {
    (void)hipFree(q);                        // the queue installed before stays in force
    return craft_host::queue_entry_invalid(bad, s->last_error);
  }
  // ticks of the old queue may still be running on some stream: they finish first
  HIP_TRY(s, hipDeviceSynchronize());
  (void)hipFree(s->d_queue);
  s->d_queue = q;
  s->q_count = count;
  (void)hipFree(s->d_tape);                  // a tape's rows mean nothing on another queue
  s->d_tape = nullptr;
  s->q_begun = false;                        // cursors of the old queue mean nothing on this one
  return CRAFT_OK;
}

int craft_episode_begin(craft_sim_t* s, int64_t first, int64_t stride, uint32_t flags, void* obs, void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_episode_begin(facts(s), first, stride, flags, obs, s->last_error)) return rc;
  const bool wrap = (flags & CRAFT_QUEUE_WRAP) != 0;
  const int64_t count = s->q_count, g0 = first + s->env_base;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const hipError_t e = craft::launch_queue_begin(s->d_queue, count, g0, wrap ? 1 : 0, s->n_envs, s->d_cursor,
                                                 s->d_qreset, st);
  if (e != hipSuccess) return hip_fail(s, e, "craft_episode_begin launch");
  const int64_t n = s->n_envs;
  const int rc = craft_reset(s, s->d_qreset, s->d_qreset + n, s->d_qreset + 2 * n, s->d_qreset + 3 * n,
                             s->d_qreset + 4 * n, obs, stream);
  if (rc != CRAFT_OK) return rc;
  s->q_step = (uint32_t)(wrap ? stride % count : std::min(stride, count));
  s->q_wrap = wrap ? 1u : 0u;
  s->q_begun = true;
  return CRAFT_OK;
}

int craft_step_stream(craft_sim_t* s, const craft_stream_step_args_t* x, void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  int rc = craft_host::check_step_stream(facts(s), x, s->last_error);
  if (rc != CRAFT_OK) return rc;
  return run_step_stream(s, x, nullptr, stream, "craft_step_stream");
}

int craft_step_lang_stream(craft_sim_t* s, const craft_lang_stream_step_args_t* x, void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_step_lang_stream(facts(s), x, s->last_error)) return rc;
  return run_step_lang_stream(s, x, nullptr, nullptr, stream, "craft_step_lang_stream");
}

int craft_step_ex(craft_sim_t* s, const craft_step_args_t* x, void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_step(x, s->last_error)) return rc;
  return run_step(s, x, nullptr, stream);
}

int craft_rollout(craft_sim_t* s, const int32_t* actions, uint64_t action_seed, int64_t tick0,
                  int32_t n_ticks, uint32_t flags, void* obs, int32_t ring, float* reward,
                  uint8_t* done, int8_t* success, void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_rollout(facts(s), tick0, n_ticks, ring, obs, s->last_error)) return rc;
  craft::RolloutArgs a{};
  a.actions = actions;
  a.seed = action_seed;
  a.tick0 = tick0;
  a.n_ticks = n_ticks;
  a.ring = ring;
  a.flags = flags;
  a.obs = obs;
  a.reward = reward;
  a.done = done;
  a.sat = success;
  a.chunk = s->k.rollout_chunk > 0 ? s->k.rollout_chunk : (n_ticks > 0 ? n_ticks : 1);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int tile = 0, threads = 0, split = 0;
  rollout_shape(s, &tile, &threads, &split);
  // chunk_ticks -1: the split kernel's continuous pipeline (its 3x3 default shape, observations
  // on; otherwise one unit per tile)
  const bool flat = s->k.rollout_chunk == -1 && split && tile == 32 && threads == 512 &&
                    s->cfg.window_width == 3 && obs != nullptr;
  a.flat = flat ? 1 : 0;
  // Chunked launches (tiles handed between workgroups) need zeroed per-tile flags.
  const int64_t n_chunks = n_ticks > 0 ? (n_ticks + a.chunk - 1) / a.chunk : 0;
  const int64_t units = ((s->n_envs + tile - 1) / tile) * n_chunks;
  bool captured = false;
  const int rc = rollout_sync(s, st, n_chunks > 1, a, captured);
  if (rc != CRAFT_OK) return rc;
  int64_t grid = 0;
  a.grid_out = &grid;
  SimView view = s->view;
  view.obs_policy = s->rollout_obs_policy;
  hipError_t e = craft::launch_rollout(s->cfg.window_width, tile, threads, view, a, lds_bytes(s, tile, 2, true), st);
  if (e != hipSuccess) return hip_fail(s, e, "craft_rollout launch");
  // the split kernel's per-unit path counts on queue[1] (craft_rollout_split.h), the others on
  // queue[0]
  if (captured) return CRAFT_OK;
  if (grid > 0 && split && !flat) s->queue1_next += (uint64_t)std::max<int64_t>(units, grid);
  else if (grid > 0) s->queue_next += (uint64_t)(units + grid);
  return CRAFT_OK;
}

int craft_rollout_stream(craft_sim_t* s, const craft_rollout_stream_args_t* x, void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  int rc = craft_host::check_rollout_stream(facts(s), x, s->last_error);
  if (rc != CRAFT_OK) return rc;
  if (x->n_ticks == 0) return CRAFT_OK;
  craft::RolloutArgs a = rollout_args(*x);
  queue_args(s, *x, a);
  // 32-env tiles; 16 where craft_sim_tune says so or where 32 envs' two staged observation
  // buffers exceed a workgroup's 160 KiB of LDS (the largest tile that fits)
  const int tile = craft::rollout_stream_tile(s->k.tile_knob, s->view);
  SimView view = s->view;
  view.obs_policy = s->rollout_obs_policy;
  return launch_tile_units(s, tile, a, stream, "craft_rollout_stream launch", [&](hipStream_t st) {
    return craft::launch_rollout_stream(s->cfg.window_width, tile, view, a, st);
  });
}

int craft_episode_actions(craft_sim_t* s, const int32_t* actions, int64_t count) {
  if (!s) return CRAFT_EINVAL;
  if (const int rc = craft_host::check_episode_actions(facts(s), actions, count, s->last_error)) return rc;
  HIP_TRY(s, hipSetDevice(s->device));
  uint8_t* tape = nullptr;
  const int T = s->cfg.max_timesteps, stride = (T + 3) & ~3;
  if (actions) {
    if (hipMalloc(&tape, (size_t)count * (size_t)stride) != hipSuccess) {
      (void)hipGetLastError();
      return fail(s, CRAFT_ENOMEM, "craft_episode_actions: out of device memory");
    }
    unsigned long long bad = ~0ull;                // (d_qbad: the queue's install allocated it)
    hipError_t e = hipMemcpy(s->d_qbad, &bad, sizeof(bad), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = craft::launch_tape_pack(actions, count, T, stride, tape, s->d_qbad, nullptr);
    if (e == hipSuccess) e = hipMemcpy(&bad, s->d_qbad, sizeof(bad), hipMemcpyDeviceToHost);   // (waits for the kernel)
    if (e != hipSuccess) {
      (void)hipFree(tape);
      return hip_fail(s, e, "craft_episode_actions");
    }
    if (bad != ~0ull) {
      (void)hipFree(tape);                         // the tape installed before stays in force
      return craft_host::tape_row_invalid(bad, s->last_error);
    }
  }
  // launches that read the old tape may still be running on some stream: they finish first
  HIP_TRY(s, hipDeviceSynchronize());
  (void)hipFree(s->d_tape);
  s->d_tape = tape;
  s->tape_stride = stride;
  return CRAFT_OK;
}

int craft_rollout_replay(craft_sim_t* s, const craft_rollout_replay_args_t* x, void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  int rc = craft_host::check_rollout_replay(facts(s), x, s->d_tape != nullptr, s->last_error);
  if (rc != CRAFT_OK) return rc;
  if (x->roll.n_ticks == 0) return CRAFT_OK;
  craft::RolloutArgs a = rollout_args(x->roll);
  queue_args(s, x->roll, a);
  a.tape = s->d_tape;
  a.tape_stride = s->tape_stride;
  a.step_now = x->step_now;
  a.act_next = x->action_next;
  const int tile = craft::rollout_stream_tile(s->k.tile_knob, s->view);
  SimView view = s->view;
  view.obs_policy = s->rollout_obs_policy;
  return launch_tile_units(s, tile, a, stream, "craft_rollout_replay launch", [&](hipStream_t st) {
    return craft::launch_rollout_replay(s->cfg.window_width, tile, view, a, st);
  });
}

int craft_rollout_teach(craft_sim_t* s, const craft_rollout_teach_args_t* x, void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  int rc = craft_host::check_rollout_teach(facts(s), x, s->last_error);
  if (rc != CRAFT_OK) return rc;
  if (x->n_ticks == 0) return CRAFT_OK;
  craft::RolloutArgs a = rollout_args(*x);
  const SimView v = teach_rollout_args(s, *x, a);
  rc = flush_table(s, stream, "craft_rollout_teach");
  if (rc != CRAFT_OK) return rc;
  return launch_tile_units(s, craft::rt_tile_of(s->cfg.window_width), a, stream, "craft_rollout_teach launch",
                           [&](hipStream_t st) {
                             return craft::launch_rollout_teach(s->cfg.window_width,
                                                                craft::teach_words(s->view.W, s->view.H), v, a, st);
                           });
}

int craft_rollout_teach_stream(craft_sim_t* s, const craft_rollout_teach_stream_args_t* x, void* stream) {
  if (!s || !x) return CRAFT_EINVAL;
  int rc = craft_host::check_rollout_teach_stream(facts(s), x, s->last_error);
  if (rc != CRAFT_OK) return rc;
  if (x->teach.n_ticks == 0) return CRAFT_OK;
  craft::RolloutArgs a = rollout_args(x->teach);
  const SimView v = teach_rollout_args(s, x->teach, a);
  queue_args(s, *x, a);
  rc = flush_table(s, stream, "craft_rollout_teach_stream");
  if (rc != CRAFT_OK) return rc;
  return launch_tile_units(s, craft::rt_tile_of(s->cfg.window_width), a, stream, "craft_rollout_teach_stream launch",
                           [&](hipStream_t st) {
                             return craft::launch_rollout_teach_stream(
                                 s->cfg.window_width, craft::teach_words(s->view.W, s->view.H), v, a, st);
                           });
}

int craft_episode_summary(craft_sim_t* s, const craft_episode_summary_args_t* x, void* stream) {
  if (!s) return CRAFT_EINVAL;
  int rc = craft_host::check_episode_summary(facts(s), x, s->last_error);
  if (rc != CRAFT_OK) return rc;
  if (x->ticks == 0) return CRAFT_OK;
  // the scan reads the teacher table for the failed get episodes: the entries of newly loaded
  // rows are built first
  if (x->distance_out) {
    rc = flush_table(s, stream, "craft_episode_summary");
    if (rc != CRAFT_OK) return rc;
  }
  const craft::SummaryArgs a{x->episode_end, x->end_pose,   x->success,     x->action_record, x->ticks,
                             x->run,         x->episode_now, s->d_queue,     s->q_count,       x->count,
                             x->length_out,  x->success_out, x->end_pose_out, x->distance_out,  x->actions_out,
                             x->flags_out};
  const hipError_t e = craft::launch_episode_summary(craft::teach_words(s->view.W, s->view.H), teach_view(s), a,
                                                     reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(s, e, "craft_episode_summary launch");
  return CRAFT_OK;
}

int craft_stats(craft_sim_t* s, int64_t* stats_out, int32_t reset, void* stream) {
  if (!s || !stats_out) return CRAFT_EINVAL;
  hipLaunchKernelGGL(craft::stats_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     s->d_stats, s->n_tiles, stats_out, (int)reset);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(s, e, "craft_stats launch");
  return CRAFT_OK;
}

int craft_transition(craft_sim_t* s, const int32_t* src, const int32_t* dst, const int32_t* actions,
                     int64_t n, int8_t* code_out, void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (n == 0) return CRAFT_OK;
  if (const int rc = craft_host::check_transition(facts(s), src, actions, n, s->last_error)) return rc;
  TileArgs a{};
  a.src = src;
  a.dst = dst;
  a.actions = actions;
  a.n = n;
  a.code = code_out;
  return launch(s, craft::MODE_TRANSITION, a, stream, "craft_transition launch");
}

int craft_observe(craft_sim_t* s, const int32_t* slots, int64_t n, const int32_t* tasks, void* obs,
                  int8_t* sat, void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (n == 0) return CRAFT_OK;
  if (const int rc = craft_host::check_observe(facts(s), slots, n, obs, s->last_error)) return rc;
  TileArgs a{};
  a.src = slots;
  a.tasks = tasks;
  a.n = n;
  a.obs = obs;
  a.sat = sat;
  return launch(s, craft::MODE_OBSERVE, a, stream, "craft_observe launch");
}

int craft_rollout_distances(craft_sim_t* s, const int32_t* tasks, const int8_t* success,
                            const int32_t* action_seqs, int32_t ticks, int32_t* distances_out,
                            uint8_t* is_get_out, int32_t* n_actions_out, int32_t* flags_out, void* stream) {
  if (!s) return CRAFT_EINVAL;
  int rc = craft_host::check_rollout_distances(facts(s), tasks, success, action_seqs, ticks, distances_out, is_get_out,
                                               n_actions_out, flags_out, s->last_error);
  if (rc != CRAFT_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(s, hipMemsetAsync(flags_out, 0, 2 * sizeof(int32_t), st));
  if (s->n_envs == 0) return CRAFT_OK;
  rc = flush_table(s, stream, "craft_rollout_distances");
  if (rc != CRAFT_OK) return rc;
  hipError_t e = craft::launch_distances(craft::teach_words(s->view.W, s->view.H), teach_view(s), tasks, success, action_seqs, ticks,
                                         s->n_envs, distances_out, is_get_out, n_actions_out, flags_out, st);
  if (e != hipSuccess) return hip_fail(s, e, "craft_rollout_distances launch");
  return CRAFT_OK;
}

int craft_teacher(craft_sim_t* s, const int32_t* slots, int64_t n, const int32_t* tasks, int32_t* action_out,
                  int32_t* path_len_out, void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (n == 0) return CRAFT_OK;
  int rc = craft_host::check_teacher(facts(s), slots, n, action_out, s->last_error);
  if (rc != CRAFT_OK) return rc;
  rc = flush_table(s, stream, "craft_teacher");
  if (rc != CRAFT_OK) return rc;
  hipError_t e = craft::launch_teacher(craft::teach_words(s->view.W, s->view.H), s->k.teach_lanes, teach_view(s), slots, tasks, n, action_out,
                                       path_len_out, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(s, e, "craft_teacher launch");
  return CRAFT_OK;
}

int craft_get_state(craft_sim_t* s, const int32_t* slots, int64_t n, int32_t* agent, int32_t* inventory,
                    uint8_t* grid, int32_t* spec, void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (n == 0) return CRAFT_OK;
  if (const int rc = craft_host::check_get_state(facts(s), slots, n, s->last_error)) return rc;
  hipLaunchKernelGGL(craft::get_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), s->view, slots, n, agent, inventory, grid, spec);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(s, e, "craft_get_state launch");
  return CRAFT_OK;
}

int craft_set_state(craft_sim_t* s, const int32_t* slots, int64_t n, const int32_t* spec, const int32_t* agent,
                    const int32_t* inventory, void* stream) {
  if (!s) return CRAFT_EINVAL;
  if (n == 0) return CRAFT_OK;
  if (const int rc = craft_host::check_set_state(facts(s), slots, n, spec, agent, s->last_error)) return rc;
  hipLaunchKernelGGL(craft::set_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), s->view, slots, n, spec, agent, inventory);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(s, e, "craft_set_state launch");
  return CRAFT_OK;
}

}  // extern "C"

#ifdef CRAFT_STAMPS
// Diagnostic builds only: route phase timestamps of the tile kernel into a
// device buffer of 8 u64 per workgroup (tools/phase_stamps.py).
extern "C" int craft_debug_set_stamps(craft_sim_t* s, uint64_t* stamps) {
  if (!s) return CRAFT_EINVAL;
  s->view.stamps = stamps;
  return CRAFT_OK;
}
#endif
