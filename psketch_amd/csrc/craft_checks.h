// craft_checks.h — what the entry points of include/craft.h refuse, and the validated tuning knobs,
// once for both libraries (craft_host.h includes this file).  Plain C++, no HIP, no handle type:
// a library fills a Facts from its own handle and calls the entry point's check before it does
// anything else.  A check returns the status and writes `msg` only when it refuses; the path that
// accepts neither allocates nor formats.  The order of the checks within an entry point is part of
// the ABI's behaviour (the first failing one names the error).
//
// The rule both libraries keep: a refused call leaves the handle as it was.  The checks read
// only; the knob setters validate every argument before they write one.
//
// Not here: `if (!s) return CRAFT_EINVAL` (no handle to record a message in), the n == 0 early
// return of the slot-list calls (not a refusal), the HIP library's own refusals (device memory,
// a stream being captured, HIP errors), errors latched per slot inside kernels and loops, and
// craft_episode_queue's per-entry validation (a kernel there, a host loop in the CPU variant:
// only its message is shared, queue_entry_invalid).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/craft.h"

namespace craft_host {

// What a check reads of a handle.
struct Facts {
  const craft_config_t* cfg;
  int64_t n_envs, env_id_base;
  int32_t pool_capacity, pool_count;
  int obs_fmt;
  int64_t queue_count;               // entries of the installed episode queue (0: none)
  bool queue_begun;                  // craft_episode_begin has run on it
};

inline int refuse(std::string& msg, int status, const char* text) {
  msg = text;
  return status;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int obs_elem_size(int fmt) { return fmt == CRAFT_OBS_F32 ? 4 : (fmt == CRAFT_OBS_BF16 ? 2 : 1); }

// Every slot of a rollout's observation ring starts 16-byte aligned (no ring: nothing to check).
inline bool ring_slots_aligned(const Facts& f, const void* obs, int ring) {
  const int64_t slot = f.n_envs * (int64_t)f.cfg->n_features * obs_elem_size(f.obs_fmt);
  return !obs || (aligned16(obs) && (ring <= 1 || slot % 16 == 0));
}

// The teachers refuse grids whose BFS would overflow the reference's 1000-state queue.
inline int bfs_queue(const Facts& f, const char* who, std::string& msg) {
  if (4 * f.cfg->width * f.cfg->height <= 1000) return CRAFT_OK;
  msg = std::string(who) + ": 4*W*H > 1000 overflows the reference's BFS queue (teachers/base.py:42)";
  return CRAFT_EINVAL;
}

// ---- the tuning knobs ---------------------------------------------------------------------------
// The tile kernel's default envs per workgroup (craft_sim_create, craft_sim_tune(0, ...)).
inline int default_tile(int win) {
  // 3x3: 64-env tiles; 5x5: 32 (35 KB of rows); 7x7: 32 (67 KB), 3 % faster than 16 at 16x16
  return win == 3 ? 64 : 32;
}

// What craft_sim_tune, craft_sim_tune_rollout, craft_sim_tune_teach and craft_sim_set_obs_format
// set (include/craft.h says what each value means).  Both handles embed one; a library applies its
// own side effects after a setter returned CRAFT_OK.
struct Knobs {
  int tile = 64;                     // envs per tile workgroup (craft_sim_create: default_tile)
  int tile_knob = 0;                 // craft_sim_tune's tile_envs as given (0 = each kernel's default)
  int resident_cap = 0;              // 0: no cap on tile workgroups per CU
  int obs_store = 2;
  int rollout_chunk = 0;             // craft_rollout ticks per work unit (0: the whole launch)
  int rollout_threads = 0;           // craft_rollout threads per tile workgroup (0: the default shape)
  int teach_kernel = 0;              // 0 auto, 1 one-tile, 2 two-tile
  int teach_lanes = 0;               // teacher lanes per query (0 = each kernel's default)
  int teach_table = 0;               // 0 auto, 1 always, 2 never
  int obs_fmt = CRAFT_OBS_F32;
};

// Whether a one-tick tile of `tile` envs fits a workgroup's 160 KiB of LDS (include/craft.h,
// craft_sim_tune): per env a grid row of ((W*H + 15) & ~15) + 4 bytes, the staged observation row
// (n_features bytes), 36 bytes of inventory and 4 of agent state; 688 bytes for the task and
// recipe tables, the subtask bytes of the teacher's tick, the control words and their 16-byte
// padding.  Never less than what craft_device.h lds_layout carves, so a tile that passes launches
// (craft_sim.hip craft_debug_tile_fits_drift checks that over the ABI's ranges).
// A 32-env tile fits every configuration the ABI admits (at most 111,824 bytes).
inline int64_t tile_lds_bound(int tile, int cells, int n_features) {
  return (int64_t)tile * (((cells + 15) & ~15) + 4 + n_features + 40) + 688;
}
inline bool tile_fits(int tile, int cells, int n_features) { return tile_lds_bound(tile, cells, n_features) <= 163840; }

inline int set_tune(Knobs& k, int win, int cells, int n_features, int32_t tile_envs, int32_t max_resident_per_cu,
                    int32_t obs_store, std::string& msg) {
  const int tile = tile_envs == 0 ? default_tile(win) : tile_envs;
  if (tile != 16 && tile != 32 && tile != 64)
    return refuse(msg, CRAFT_EINVAL, "craft_sim_tune: tile_envs must be 16, 32 or 64");
  if (!tile_fits(tile, cells, n_features))
    return refuse(msg, CRAFT_EINVAL,
                  "craft_sim_tune: a tile of tile_envs envs does not fit a workgroup's 160 KiB of LDS with this window and kind count");
  if (max_resident_per_cu != 0 && (max_resident_per_cu < 3 || max_resident_per_cu > 32))
    return refuse(msg, CRAFT_EINVAL, "craft_sim_tune: max_resident_per_cu must be 0 or 3..32");
  if (obs_store < 0 || obs_store > 2)
    return refuse(msg, CRAFT_EINVAL,
                  "craft_sim_tune: obs_store must be 0 (write-back), 1 (nontemporal) or 2 (write-through)");
  k.tile_knob = tile_envs;
  k.tile = tile;
  k.resident_cap = max_resident_per_cu;
  k.obs_store = obs_store;
  return CRAFT_OK;
}

inline int set_tune_teach(Knobs& k, int32_t kernel, int32_t lanes, int32_t table, std::string& msg) {
  if (kernel < 0 || kernel > 2)
    return refuse(msg, CRAFT_EINVAL, "craft_sim_tune_teach: kernel must be 0 (auto), 1 (one-tile) or 2 (two-tile)");
  if (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 4)
    return refuse(msg, CRAFT_EINVAL, "craft_sim_tune_teach: lanes must be 0 (default), 1, 2 or 4");
  if (table < 0 || table > 2)
    return refuse(msg, CRAFT_EINVAL, "craft_sim_tune_teach: table must be 0 (auto), 1 (always) or 2 (never)");
  k.teach_kernel = kernel;
  k.teach_lanes = lanes;
  k.teach_table = table;
  return CRAFT_OK;
}

inline int set_tune_rollout(Knobs& k, int32_t chunk_ticks, int32_t threads, std::string& msg) {
  if (chunk_ticks < -1 || chunk_ticks > 4096)
    return refuse(msg, CRAFT_EINVAL, "craft_sim_tune_rollout: chunk_ticks must be -1..4096");
  if (threads != 0 && threads != 128 && threads != 256 && threads != 320 && threads != 384 && threads != 512)
    return refuse(msg, CRAFT_EINVAL, "craft_sim_tune_rollout: threads must be 0, 128, 256, 320, 384 or 512");
  k.rollout_chunk = chunk_ticks;
  k.rollout_threads = threads;
  return CRAFT_OK;
}

inline int set_obs_format(Knobs& k, int32_t format, std::string& msg) {
  if (format != CRAFT_OBS_F32 && format != CRAFT_OBS_BF16 && format != CRAFT_OBS_U8)
    return refuse(msg, CRAFT_EINVAL, "craft_sim_set_obs_format: format must be 0 (fp32), 1 (bf16) or 2 (u8)");
  k.obs_fmt = format;
  return CRAFT_OK;
}

// craft_sim_tune_host's threads (the CPU variant keeps them; the HIP library has no host workers).
inline int check_tune_host(int32_t threads, std::string& msg) {
  if (threads < 0 || threads > 1024)
    return refuse(msg, CRAFT_EINVAL, "craft_sim_tune_host: threads must be 0 (the machine's) or 1..1024");
  return CRAFT_OK;
}

// ---- the scenario pool --------------------------------------------------------------------------
// (each grid of craft_pool_load: check_pool_grid, craft_host.h)
inline int check_pool_load(const Facts& f, const uint8_t* grids, int32_t first, int32_t count, std::string& msg) {
  if (!grids || first < 0 || count < 0) return refuse(msg, CRAFT_EINVAL, "craft_pool_load: bad argument");
  if ((int64_t)first + count > f.pool_capacity)
    return refuse(msg, CRAFT_ERANGE, "craft_pool_load: beyond pool capacity");
  return CRAFT_OK;
}

inline int check_pool_generate(const Facts& f, int32_t first, int32_t count, int32_t boundary_kind,
                               const int32_t* primitives, int32_t n_primitive_kinds, int32_t n_per_primitive,
                               const int32_t* workshop_kind, int32_t n_workshops, std::string& msg) {
  if (first < 0 || count < 0 || n_primitive_kinds < 0 || n_primitive_kinds > 8 || n_per_primitive < 0 ||
      n_workshops < 0 || n_workshops > 8 || (n_primitive_kinds && !primitives) || (n_workshops && !workshop_kind))
    return refuse(msg, CRAFT_EINVAL, "craft_pool_generate: bad argument");
  if ((int64_t)first + count > f.pool_capacity)
    return refuse(msg, CRAFT_ERANGE, "craft_pool_generate: beyond pool capacity");
  const int K = f.cfg->n_kinds, W = f.cfg->width, H = f.cfg->height;
  auto bad_kind = [&](int k) { return k <= 0 || k >= K; };
  if (bad_kind(boundary_kind)) return refuse(msg, CRAFT_EINVAL, "craft_pool_generate: bad boundary kind");
  for (int i = 0; i < n_primitive_kinds; ++i)
    if (bad_kind(primitives[i])) return refuse(msg, CRAFT_EINVAL, "craft_pool_generate: bad primitive kind");
  for (int i = 0; i < n_workshops; ++i)
    if (bad_kind(workshop_kind[i])) return refuse(msg, CRAFT_EINVAL, "craft_pool_generate: bad workshop kind");
  if ((int64_t)n_primitive_kinds * n_per_primitive + n_workshops + 1 > (int64_t)(W - 2) * (H - 2))
    return refuse(msg, CRAFT_EINVAL, "craft_pool_generate: more objects than interior cells");
  return CRAFT_OK;
}

// ---- reset and the ticks ------------------------------------------------------------------------
inline int check_reset(const int32_t* scenario, const int32_t* pos_x, const int32_t* pos_y, const int32_t* dir,
                       const int32_t* task, const void* obs, std::string& msg) {
  if (!scenario || !pos_x || !pos_y || !dir || !task) return refuse(msg, CRAFT_EINVAL, "craft_reset: null input");
  if (obs && !aligned16(obs)) return refuse(msg, CRAFT_EINVAL, "craft_reset: obs must be 16-byte aligned");
  return CRAFT_OK;
}

// craft_step / craft_step_ex, and the craft_step_args_t of craft_step_teach and craft_step_stream.
inline int check_step(const craft_step_args_t* x, std::string& msg) {
  if (x->obs && !aligned16(x->obs)) return refuse(msg, CRAFT_EINVAL, "craft_step: obs must be 16-byte aligned");
  if (x->behavior_clone && !x->ref_actions)
    return refuse(msg, CRAFT_EINVAL, "craft_step_ex: behavior_clone needs ref_actions");
  return CRAFT_OK;
}

inline int check_step_teach(const Facts& f, const craft_step_args_t* x, std::string& msg) {
  if (const int rc = bfs_queue(f, "craft_step_teach", msg)) return rc;
  return check_step(x, msg);
}

inline int check_step_lang(const Facts& f, const craft_lang_step_args_t* x, std::string& msg) {
  if (x->flags != 0)
    return refuse(msg, CRAFT_EINVAL, "craft_step_lang: flags must be 0 (no auto-reset in this protocol)");
  if (x->use_alt && !x->alt_actions) return refuse(msg, CRAFT_EINVAL, "craft_step_lang: use_alt needs alt_actions");
  if (x->obs && !aligned16(x->obs)) return refuse(msg, CRAFT_EINVAL, "craft_step_lang: obs must be 16-byte aligned");
  return x->label_out ? bfs_queue(f, "craft_step_lang", msg) : CRAFT_OK;
}

// ---- the episode queue --------------------------------------------------------------------------
inline int check_episode_queue(const int32_t* specs, int64_t count, std::string& msg) {
  if (!specs || count < 1 || count > (int64_t)INT32_MAX)
    return refuse(msg, CRAFT_EINVAL, "craft_episode_queue: specs must hold 1 .. 2^31 - 1 entries");
  return CRAFT_OK;
}

// craft_episode_queue's refusal of a queue whose lowest invalid entry is `index`.
inline int queue_entry_invalid(uint64_t index, std::string& msg) {
  msg = "craft_episode_queue: entry " + std::to_string(index) +
        " is invalid (scenario, position, direction or task out of range)";
  return CRAFT_EINVAL;
}

inline int check_episode_begin(const Facts& f, int64_t first, int64_t stride, uint32_t flags, const void* obs,
                               std::string& msg) {
  if (f.queue_count == 0)
    return refuse(msg, CRAFT_EINVAL, "craft_episode_begin: no episode queue installed (craft_episode_queue)");
  if (stride < 1) return refuse(msg, CRAFT_EINVAL, "craft_episode_begin: stride must be >= 1");
  if (first < 0) return refuse(msg, CRAFT_EINVAL, "craft_episode_begin: first must be >= 0");
  if (flags & ~CRAFT_QUEUE_WRAP) return refuse(msg, CRAFT_EINVAL, "craft_episode_begin: unknown flag");
  if (obs && !aligned16(obs)) return refuse(msg, CRAFT_EINVAL, "craft_episode_begin: obs must be 16-byte aligned");
  if (first > INT64_MAX - f.env_id_base - f.n_envs)
    return refuse(msg, CRAFT_EINVAL, "craft_episode_begin: first is out of range");
  const int64_t g0 = first + f.env_id_base, count = f.queue_count;
  if (!(flags & CRAFT_QUEUE_WRAP) && f.n_envs > 0 && g0 + f.n_envs - 1 >= count) {
    msg = "craft_episode_begin: slot " + std::to_string(std::max<int64_t>(count - g0, 0)) +
          " would start past the end of the queue (" + std::to_string(count) + " entries)";
    return CRAFT_EINVAL;
  }
  return CRAFT_OK;
}

inline int check_step_stream(const Facts& f, const craft_stream_step_args_t* x, std::string& msg) {
  if (x->step.flags != CRAFT_STEP_AUTORESET)
    return refuse(msg, CRAFT_EINVAL, "craft_step_stream: step.flags must be CRAFT_STEP_AUTORESET");
  if (f.queue_count == 0 || !f.queue_begun)
    return refuse(msg, CRAFT_EINVAL, "craft_step_stream: craft_episode_begin has not put the slots on the queue");
  if (x->label_out)
    if (const int rc = bfs_queue(f, "craft_step_stream", msg)) return rc;
  return check_step(&x->step, msg);
}

// ---- the multi-tick launches --------------------------------------------------------------------
inline int check_rollout(const Facts& f, int64_t tick0, int32_t n_ticks, int32_t ring, const void* obs,
                         std::string& msg) {
  if (n_ticks < 0 || ring < 1 || tick0 < 0)
    return refuse(msg, CRAFT_EINVAL, "craft_rollout: need n_ticks >= 0, ring >= 1, tick0 >= 0");
  if (!ring_slots_aligned(f, obs, ring))
    return refuse(msg, CRAFT_EINVAL, "craft_rollout: every obs ring slot must be 16-byte aligned");
  return CRAFT_OK;
}

inline int check_rollout_teach(const Facts& f, const craft_rollout_teach_args_t* x, std::string& msg) {
  if (x->n_ticks < 0 || x->ring < 1 || x->tick0 < 0)
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_teach: need n_ticks >= 0, ring >= 1, tick0 >= 0");
  if (const int rc = bfs_queue(f, "craft_rollout_teach", msg)) return rc;
  if ((x->label_actions != 0 || x->behavior_clone != nullptr) && !x->label_in)
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_teach: label_actions / behavior_clone need label_in");
  if (!ring_slots_aligned(f, x->obs, x->ring))
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_teach: every obs ring slot must be 16-byte aligned");
  return CRAFT_OK;
}

inline int check_rollout_distances(const Facts& f, const int32_t* tasks, const int8_t* success,
                                   const int32_t* action_seqs, int32_t ticks, const int32_t* distances_out,
                                   const uint8_t* is_get_out, const int32_t* n_actions_out,
                                   const int32_t* flags_out, std::string& msg) {
  if (!tasks || !success || !distances_out || !is_get_out || !n_actions_out || !flags_out || ticks < 0 ||
      (ticks > 0 && !action_seqs))
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_distances: bad argument");
  return bfs_queue(f, "craft_rollout_distances", msg);
}

// ---- the slot-list calls (n items; a null slot list means slots 0 .. n-1) -------------------------
inline int check_transition(const Facts& f, const int32_t* src, const int32_t* actions, int64_t n, std::string& msg) {
  if (!actions || n < 0) return refuse(msg, CRAFT_EINVAL, "craft_transition: bad argument");
  if (!src && n > f.n_envs) return refuse(msg, CRAFT_ERANGE, "craft_transition: n > n_envs");
  return CRAFT_OK;
}

inline int check_observe(const Facts& f, const int32_t* slots, int64_t n, const void* obs, std::string& msg) {
  if (n < 0) return refuse(msg, CRAFT_EINVAL, "craft_observe: bad argument");
  if (!slots && n > f.n_envs) return refuse(msg, CRAFT_ERANGE, "craft_observe: n > n_envs");
  if (obs && !aligned16(obs)) return refuse(msg, CRAFT_EINVAL, "craft_observe: obs must be 16-byte aligned");
  return CRAFT_OK;
}

inline int check_teacher(const Facts& f, const int32_t* slots, int64_t n, const int32_t* action_out,
                         std::string& msg) {
  if (!action_out || n < 0) return refuse(msg, CRAFT_EINVAL, "craft_teacher: bad argument");
  if (!slots && n > f.n_envs) return refuse(msg, CRAFT_ERANGE, "craft_teacher: n > n_envs");
  return bfs_queue(f, "craft_teacher", msg);
}

inline int check_get_state(const Facts& f, const int32_t* slots, int64_t n, std::string& msg) {
  if (n < 0) return refuse(msg, CRAFT_EINVAL, "craft_get_state: bad argument");
  if (!slots && n > f.n_envs) return refuse(msg, CRAFT_ERANGE, "craft_get_state: n > n_envs");
  return CRAFT_OK;
}

inline int check_set_state(const Facts& f, const int32_t* slots, int64_t n, const int32_t* spec,
                           const int32_t* agent, std::string& msg) {
  if (n < 0 || !spec || !agent) return refuse(msg, CRAFT_EINVAL, "craft_set_state: bad argument");
  if (!slots && n > f.n_envs) return refuse(msg, CRAFT_ERANGE, "craft_set_state: n > n_envs");
  return CRAFT_OK;
}

}  // namespace craft_host
