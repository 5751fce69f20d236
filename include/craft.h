/*
 * craft.h — C ABI of the MI355X-native batched CraftWorld simulator.
 *
 * The reference (khanhptnk/psketch) has no FFI: its boundary is the Python
 * duck-typed world protocol selected by name in worlds/__init__.py:5-11
 * (`globals()[config.world.name](config)`).  Every entry point below replaces
 * one piece of that protocol, batched over N environments that live as
 * struct-of-arrays in HBM.  The Python host side (psketch_amd/) binds these
 * with ctypes; INTEGRATION.md shows the binding a maintainer adds to the
 * reference.
 *
 * Conventions
 *   - Plain C types only.  `stream` is a hipStream_t passed as void* (NULL =
 *     the null stream).  Pointers documented "device" are HBM pointers owned by
 *     the caller; "host" pointers are host memory owned by the caller.
 *   - Every function returns a craft_status (0 = CRAFT_OK).  A failing call
 *     stores a message retrievable with craft_sim_last_error().
 *   - Kernel-side errors (an out-of-range action, a teacher assertion) cannot
 *     be returned synchronously; they latch in a device error word that
 *     craft_sim_check() reads (it synchronises the stream).
 *   - A handle is not thread-safe; calls are stream-ordered.  No allocation
 *     happens on the step path.
 *
 * Grid convention: cell (x, y) of a W x H world is index x*H + y (x-major),
 * exactly the order of `grid[x, y, :]` in worlds/craft.py and of
 * `np.nonzero` in CraftState.find_resource_positions (craft.py:453-455).
 * A cell holds one kind id (0 = empty); the reference's one-hot W x H x K
 * float64 grid maps 1:1 onto it (its one-kind-per-cell invariant is asserted
 * at craft.py:365-371 and checked when a grid is loaded).
 */
#ifndef PSKETCH_CRAFT_H
#define PSKETCH_CRAFT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: craft_sim_tune_teach takes (kernel, lanes, table) (was (kernel)); craft_sim_tune_host,
 * craft_sim_sync_table and craft_abi_version added. */
#define CRAFT_ABI_VERSION 2

#define CRAFT_MAX_KINDS 32       /* len(cookbook.index) incl. reserved 0 (21 for recipes.yaml) */
#define CRAFT_MAX_RECIPES 16     /* recipes.yaml has 9 */
#define CRAFT_MAX_INGREDIENTS 4
#define CRAFT_MAX_TASKS 64       /* hints.hierarchy.yaml has 26 */
#define CRAFT_MAX_SUBTASKS 4
#define CRAFT_MAX_DIM 16         /* W, H <= 16 */
#define CRAFT_MAX_CELLS 256      /* W * H <= 256 */

/* status codes */
typedef enum craft_status {
  CRAFT_OK = 0,
  CRAFT_EINVAL = 1,       /* bad argument / configuration */
  CRAFT_EBADACTION = 2,   /* action outside 0..5: craft.py:415-416 `Exception("Unexpected action")` */
  CRAFT_EINVARIANT = 3,   /* grid breaks an invariant: craft.py:365-371 AssertionError */
  CRAFT_ETEACHER = 4,     /* teacher assertion / crash: teachers/base.py:24,31; demonstration.py:18 */
  CRAFT_EHIP = 5,         /* HIP runtime failure */
  CRAFT_ENOMEM = 6,
  CRAFT_ERANGE = 7        /* slot / scenario index out of range */
} craft_status;

/* Actions, craft.py:25-31.  Moves use world.actions.*.coord_change, craft.py:77-91. */
enum {
  CRAFT_DOWN = 0,   /* (0, -1) */
  CRAFT_UP = 1,     /* (0, +1) */
  CRAFT_LEFT = 2,   /* (-1, 0) */
  CRAFT_RIGHT = 3,  /* (+1, 0) */
  CRAFT_USE = 4,
  CRAFT_STOP = 5,
  CRAFT_N_ACTIONS = 6
};

/* What USE does to a facing cell holding a kind (craft.py:373-410, 101-107). */
enum {
  CRAFT_KIND_INERT = 0,      /* boundary, or a workshop index >= N_WORKSHOPS: USE is a no-op */
  CRAFT_KIND_GRABBABLE = 1,  /* not in cookbook.environment: inventory += 1, cell cleared */
  CRAFT_KIND_WORKSHOP = 2,   /* workshop0..N_WORKSHOPS-1: apply its recipes in dict order */
  CRAFT_KIND_WATER = 3,      /* with bridge > 0: cell cleared, bridge -= 1 */
  CRAFT_KIND_STONE = 4       /* with axe > 0: cell cleared, axe kept */
};

/* Task.goal_name values (data/task.py:11) that CraftState.satisfies and the
 * DemonstrationTeacher distinguish (craft.py:285-294, teachers/demonstration.py:18-21). */
enum {
  CRAFT_GOAL_OTHER = 0,   /* left/right/up/down/stop/makeat: satisfies() -> None */
  CRAFT_GOAL_GET = 1,     /* inventory[arg] > 0 */
  CRAFT_GOAL_MAKE = 2,    /* inventory[arg] > 0 */
  CRAFT_GOAL_GO = 3,      /* facing cell holds arg */
  CRAFT_GOAL_USE = 4      /* satisfies() -> None; teacher leaf -> USE */
};

typedef struct craft_recipe {
  int32_t output;        /* kind id produced */
  int32_t workshop;      /* kind id of its `_at` workshop */
  int32_t yield;         /* `_yield`, default 1, 1..255 (craft.py:394); a u8 count that would pass
                            255 saturates and latches CRAFT_ERANGE */
  int32_t n_inputs;
  int32_t input_kind[CRAFT_MAX_INGREDIENTS];
  int32_t input_count[CRAFT_MAX_INGREDIENTS];
} craft_recipe_t;

typedef struct craft_task {
  int32_t goal;          /* CRAFT_GOAL_* */
  int32_t arg_kind;      /* cookbook.index[goal_arg]; 0 when the arg is not a kind */
  int32_t n_subtasks;    /* 0 = leaf (data/task.py:13-15) */
  int32_t subtask[CRAFT_MAX_SUBTASKS];   /* task ids, in hint order */
} craft_task_t;

/* Static world tables: CraftWorld.__init__ (craft.py:59-109), Cookbook
 * (worlds/cookbook.py:8-26), TaskManager (data/task.py:32-75). */
typedef struct craft_config {
  int32_t abi_version;       /* = CRAFT_ABI_VERSION */
  int32_t width, height;     /* WIDTH, HEIGHT: independent (3..16 each, width*height <= 256; cells are
                              * x*height + y).  The teacher entry points refuse 4*W*H > 1000, so
                              * 15x16 and 16x15 are the largest worlds they label. */
  int32_t window_width, window_height;   /* WINDOW_WIDTH, WINDOW_HEIGHT (odd, equal, 3..7) */
  int32_t n_kinds;           /* len(cookbook.index) */
  int32_t n_features;        /* must equal 2*ww*wh*n_kinds + n_kinds + 5 (craft.py:69-75) */
  int32_t max_timesteps;     /* trainer.max_timesteps (configs/experiments/imitation.yaml:21) */
  int32_t bridge_kind, axe_kind;
  uint8_t kind_class[CRAFT_MAX_KINDS];   /* CRAFT_KIND_* per kind id */
  int32_t n_recipes;
  craft_recipe_t recipe[CRAFT_MAX_RECIPES];   /* cookbook.recipes in dict (YAML) order */
  int32_t n_tasks;
  craft_task_t task[CRAFT_MAX_TASKS];         /* TaskManager.tasks order */
} craft_config_t;

typedef struct craft_sim craft_sim_t;

/* ---- handle lifetime ------------------------------------------------------ */

/* CRAFT_ABI_VERSION of the loaded library: a caller that binds the symbols at run time (dlsym,
 * ctypes) checks it before calling anything whose signature changed between versions. */
int craft_abi_version(void);

/* Replaces CraftWorld.__init__ (craft.py:59-109) for a batch of `n_envs`
 * environment slots on `device`.  `env_id_base` is the global id of slot 0
 * (rank * n_envs when sharded): per-env randomness is keyed by global id so
 * results do not depend on the number of GPUs.  `pool_capacity` scenario
 * grids can be loaded. */
int craft_sim_create(const craft_config_t* cfg, int device, int64_t n_envs,
                     int64_t env_id_base, int32_t pool_capacity, craft_sim_t** out);
int craft_sim_destroy(craft_sim_t* sim);
const char* craft_sim_last_error(const craft_sim_t* sim);
const char* craft_strerror(int status);
int craft_sim_info(const craft_sim_t* sim, int64_t* n_envs, int32_t* pool_capacity,
                   int32_t* n_features);

/* Performance knobs of the tile kernels (results are identical for every
 * setting): envs per workgroup tile (16, 32 or 64; 0 = default for the
 * window), the most tile workgroups that may share a CU (0 = no cap, else
 * 3..32), and the cache policy of the observation stores (0 write-back,
 * 1 nontemporal, 2 write-through) for every entry point.  Until it is called,
 * every kernel stores write-through (sc1; the measured best for craft_rollout and for a
 * tick that rewrites one buffer) except craft_rollout_teach, which stores nontemporal (its
 * teacher-table gathers keep their L2 lines: 7-15 % faster at 65,536 envs).
 * Note: craft_sim_tune(.., 0, 0, 0) selects write-back.
 * CRAFT_EINVAL, and the handle keeps its knobs: a value outside the ranges above, or a tile whose
 * one-tick working set does not fit a workgroup's 160 KiB of LDS, that is
 *   tile_envs * (((WIDTH*HEIGHT + 15) & ~15) + n_features + 44) + 688 > 163840
 * (64-env tiles at 7x7 windows, from 23 kinds on the largest worlds; a 32-env tile always fits).  Both libraries refuse
 * it, so no tick ever launches a tile that cannot be carved; where craft_step_teach's one-tile
 * kernel would pick 64-env tiles of its own that do not fit, it runs 32-env tiles
 * (craft_sim_step_shape reports them). */
int craft_sim_tune(craft_sim_t* sim, int32_t tile_envs, int32_t max_resident_per_cu,
                   int32_t obs_store);

/* craft_rollout scheduling knobs (results are identical for every setting).
 * chunk_ticks: work-unit length.  The launch is cut into (tile, chunk of
 * chunk_ticks ticks) units handed out dynamically to the workgroups, a tile's
 * state passing between workgroups at chunk boundaries, so slow workgroups do
 * fewer units.  0 (default) = one unit per tile for the whole launch, which
 * measured fastest at 65536 envs (the balance gained does not pay for the
 * hand-offs).  -1 = one continuous pipeline per workgroup across
 * the tiles it claims (no pipeline fill and drain per tile, the next tile
 * prefetched by LDS-DMA; the split kernel's 3x3 default shape only): measured
 * level with 0.  threads: threads per tile workgroup on the tile
 * set by craft_sim_tune.  128 or 256: one producer wave, the rest stream; 64-env
 * tiles also take 512.  16- and 32-env tiles with 320, 384 or 512: the
 * split-producer kernel (transition and scatter on two waves, the other 3-6
 * stream).  0 (default) = the measured best: 32-env tiles x 512 threads (split)
 * for 3x3 windows, else the handle's tile with 256 threads (512 for 64-env tiles).  A tile whose
 * two staged observation buffers do not fit a workgroup's 160 KiB of LDS (64 envs at 7x7 windows)
 * runs as the largest tile that does; craft_sim_rollout_shape reports it. */
int craft_sim_tune_rollout(craft_sim_t* sim, int32_t chunk_ticks, int32_t threads);

/* The teacher's knobs (results are identical for every setting; a tuning knob like
 * craft_sim_tune, replacing nothing in the reference):
 *   kernel  which kernel craft_step_teach launches: 0 (default) = the measured best (the two-tile
 *           kernel with 2 teacher lanes per env for 3x3 windows at >= 32768 envs, else the
 *           one-tile kernel: 64-env tiles with 4 lanes for 3x3 windows, the handle's tile (32
 *           by default) with 2 for wider ones), 1 = the one-tile kernel, 2 = the two-tile
 *           kernel (3x3 windows and the default tile only; otherwise the one-tile kernel);
 *   lanes   teacher lanes per query: 0 (default) = each kernel's measured best; 1, 2 or 4 for
 *           craft_teacher and the one-tile kernel, 2 or 4 for the two-tile kernel (others: 2);
 *   table   which teachers read the teacher table (find_closest_resources answered ahead of
 *           time for every grid an env can reach: its pool row minus any subset of the row's
 *           first m clearable cells (m <= 8), for every go/get target kind, start cell and
 *           direction; 4*W*H u16 entries per kind per (row, subset), allocated at the first pool
 *           load for pool_capacity rows with m chosen to fit 1 GiB (12x12 craft_medium: m = 6,
 *           453 MB for 1024 rows); a loaded row's entries are built by the next launch that reads
 *           the table, on its stream, which then waits for them (craft_sim_sync_table)), for envs
 *           whose grid it lists: 0 (default) = auto (every teacher: measured faster in every
 *           launch shape since the 4-bit copy), 1 = always, 2 = never (every query runs the BFS). */
int craft_sim_tune_teach(craft_sim_t* sim, int32_t kernel, int32_t lanes, int32_t table);

/* Host worker threads of the CPU variant of this ABI (libpsketch_craft_cpu.so), which splits
 * every batched call over contiguous slot ranges: 0 = the machine's hardware threads (the
 * default), else 1..1024.  Results are identical for every setting.  The HIP library runs no
 * host workers: it validates the argument and keeps nothing. */
int craft_sim_tune_host(craft_sim_t* sim, int32_t threads);

/* Builds, on `stream`, the teacher-table entries of the pool rows craft_pool_load has loaded since
 * the last build, and waits for them.  Every launch that reads the table (craft_step_teach,
 * craft_rollout_teach, craft_teacher, craft_rollout_distances) does this first, so a caller needs
 * it only before capturing such a launch into a HIP graph right after a pool load: a launch
 * being captured refuses (CRAFT_EINVAL) to build them.  No-op when nothing is pending. */
int craft_sim_sync_table(craft_sim_t* sim, void* stream);

/* The kernel craft_step / craft_step_ex (teach == 0) or craft_step_teach (teach != 0) will
 * launch, resolved from the knobs above: *kernel = CRAFT_KERNEL_TILE / _TICK2, *envs =
 * envs per tile (tile kernel) or per workgroup (two-tile kernel),
 * *lanes = teacher lanes per env (0 without a teacher).  Lets a caller (bench.py) name the
 * kernel it times instead of mirroring the library's defaults. */
#define CRAFT_KERNEL_TILE 1
#define CRAFT_KERNEL_TICK2 2
int craft_sim_step_shape(const craft_sim_t* sim, int32_t teach, int32_t* kernel, int32_t* envs,
                         int32_t* lanes);

/* The launch shape the next craft_rollout will use, resolved from the knobs above:
 * envs per tile workgroup, threads per workgroup, and split = 1 for the
 * split-producer kernel (rollout_split_kernel), 0 for rollout_kernel.  Lets a
 * caller (bench.py) name the kernel it times instead of mirroring the defaults. */
int craft_sim_rollout_shape(const craft_sim_t* sim, int32_t* tile_envs, int32_t* threads,
                            int32_t* split);

/* The tile kernel's current envs per workgroup and observation store policy
 * (craft_sim_tune), for the same purpose on the craft_step path. */
int craft_sim_tile_shape(const craft_sim_t* sim, int32_t* tile_envs, int32_t* obs_store);

/* Element type of every observation buffer this handle writes (craft_reset,
 * craft_step, craft_step_ex, craft_observe).  The features are small
 * non-negative integers (one-hots, block maxima, inventory counts < 256), so
 * all three formats hold exactly the reference's values; bf16 and u8 cut the
 * observation stream (the kernel's dominant HBM traffic) by 2x and 4x for a
 * student that consumes them directly.  Default CRAFT_OBS_F32. */
typedef enum {
  CRAFT_OBS_F32 = 0,
  CRAFT_OBS_BF16 = 1,
  CRAFT_OBS_U8 = 2
} craft_obs_format_t;
int craft_sim_set_obs_format(craft_sim_t* sim, int32_t format);

/* Synchronises `stream` and returns the first kernel-side error latched since
 * the last call (then clears it); *env_out receives the offending slot. */
int craft_sim_check(craft_sim_t* sim, int64_t* env_out, void* stream);

/* Without synchronising: queues a copy of the latched-error record into device int32[4]
 * `out` on `stream` ({status, 0, slot low, slot high}; status 0 = no error), so a caller can
 * read it back together with its own results and call craft_sim_check only when it is set. */
int craft_sim_error_word(craft_sim_t* sim, int32_t* out, void* stream);

/* ---- scenario pool ---------------------------------------------------------- */

/* Uploads `count` initial grids (host, count * W*H kind ids, x-major) into pool
 * entries [first, first+count).  Replaces the `grid` handed to
 * CraftWorld.init_state (craft.py:258-259).  Rejects (CRAFT_EINVARIANT) kind ids
 * >= n_kinds and worlds whose border ring holds a cell that is empty, not inert
 * (CRAFT_KIND_INERT: USE could clear it) or some task's target kind: every
 * make_data.py world has the boundary ring (make_data.py:108-112), and the
 * teacher's BFS and the kernels rely on it. Synchronous. */
int craft_pool_load(craft_sim_t* sim, const uint8_t* grids, int32_t first, int32_t count);

/* ---- episodes ---------------------------------------------------------------- */

/* CraftScenario.init (craft.py:262-273) for every slot: inventory zeroed,
 * grid = pool[scenario], pos/dir given, timer = max_timesteps.  The spec is
 * kept so that an auto-reset returns the slot to the same initial state.
 * Device arrays of n_envs int32 each; `obs` (n_envs x n_features, obs format) may be
 * NULL, else receives features() of the initial states. */
int craft_reset(craft_sim_t* sim, const int32_t* scenario, const int32_t* pos_x,
                const int32_t* pos_y, const int32_t* dir, const int32_t* task,
                void* obs, void* stream);

#define CRAFT_STEP_AUTORESET 1u   /* done slots restart from their spec next tick */

/* One tick of the imitation-trainer rollout for every slot, fused with the
 * observation: the per-env body of ImitationTrainer.do_rollout
 * (trainers/imitation.py:59-73) followed by CraftState.features() of the new
 * state (craft.py:296-330).
 *   timer -= 1; done = (a == STOP) or timer <= 0
 *   done  -> success = satisfies(task) on the pre-step state, no step
 *            (auto-reset: the slot restarts; else it stays frozen)
 *   !done -> state = step(state, a)            (craft.py:332-424)
 * `actions` (device int32[n_envs]) may be NULL: actions are then drawn in the
 * kernel as splitmix64(action_seed ^ (gid << 20) ^ tick) >> 32 mod 6.
 * Outputs (device, each may be NULL): obs [n_envs][n_features] (obs format);
 * reward fp32 (1 on a tick that ends an episode with satisfies() true, else 0 —
 * step() itself always returns 0, craft.py:338); done uint8; success int8
 * (-1 not terminal, else satisfies()).  Episode statistics accumulate inside
 * the handle (per-workgroup partial sums, no atomics); read them with
 * craft_stats. */
int craft_step(craft_sim_t* sim, const int32_t* actions, uint64_t action_seed, int64_t tick,
               uint32_t flags, void* obs, float* reward, uint8_t* done, int8_t* success,
               void* stream);

/* craft_step with the rest of a do_rollout tick fused in (trainers/imitation.py:43-73):
 *   a = behavior_clone[i] ? ref_actions[i] : actions[i]     (imitation.py:56-57)
 *   action_record[i] = a, or -1 for a slot already done     (action_seqs, :59-61)
 *   *any_live = 1 if some slot is still running after this tick (all(done), :42)
 * then the craft_step tick.  ref_actions is craft_teacher's output for the same
 * slots (a done slot's label is -1 and is never used).  Every pointer may be
 * NULL: actions NULL = the hashed draw; ref_actions/behavior_clone NULL = no
 * cloning.  any_live is a device int32 the kernel only ever sets to 1 (plain
 * stores, no atomics: point it at element t of a zeroed per-tick array).  The
 * rollout counters come from craft_stats: num_interactions (:54) = env-steps,
 * num_steps (:71) = env-steps - episodes ended.  obs has the handle's obs format. */
typedef struct {
  const int32_t* actions;          /* int32[n_envs] student actions */
  const int32_t* ref_actions;      /* int32[n_envs] teacher labels */
  const uint8_t* behavior_clone;   /* uint8[n_envs] 0/1 */
  uint64_t action_seed;
  int64_t tick;
  uint32_t flags;                  /* CRAFT_STEP_AUTORESET */
  void* obs;                       /* [n_envs][n_features] in the obs format */
  float* reward;
  uint8_t* done;
  int8_t* success;
  int32_t* action_record;          /* int32[n_envs] */
  int32_t* any_live;               /* int32 scalar flag */
  int8_t* transition_code;         /* int8[n_envs]: see craft_transition; -1 if no step */
} craft_step_args_t;
int craft_step_ex(craft_sim_t* sim, const craft_step_args_t* args, void* stream);

/* The device address of page-locked host memory (hipHostGetDevicePointer), e.g. for an
 * any_live flag array the host polls after an event instead of copying each tick's flag
 * back (the kernel's plain stores of 1 are visible to the host once the launch has
 * completed).  CRAFT_EINVAL if `host` is not page-locked memory HIP maps. */
int craft_host_flag_pointer(void* host, int32_t** device_out);

/* craft_step_ex fused with craft_teacher on every slot's NEW state (its own task),
 * in one launch: label_out (device int32[n_envs]) receives
 * DemonstrationTeacher.__call__ (teachers/demonstration.py:9-30) of each slot
 * after the tick — the ref_actions of the next tick of ImitationTrainer.do_rollout
 * (trainers/imitation.py:47-55): -1 for a slot the tick left frozen, -2 (and
 * CRAFT_ETEACHER latched) where the reference raises.  Identical to craft_step_ex
 * followed by craft_teacher(slots NULL, tasks NULL), but the teacher reads the
 * grid rows the tick holds on chip instead of rebuilding them from HBM, and its
 * BFS overlaps the observation stores (config 5: a teacher label every tick). */
int craft_step_teach(craft_sim_t* sim, const craft_step_args_t* args, int32_t* label_out, void* stream);

/* One tick of the language trainers' rollout, in one launch: the per-env body of the loop the
 * reference's PrimitiveLanguageTrainer, InteractivePrimitiveLanguageTrainer and
 * ActivePrimitiveLanguageTrainer share (trainers/primitive_language.py:45-66,
 * interactive_primitive_language.py:43-76, active_primitive_language.py:44-87), fused with
 * features() of the new state and, with label_out, the DemonstrationTeacher on it.  Unlike
 * craft_step's protocol the step comes first.  Per slot, in this order:
 *   a slot frozen before the tick takes no step and leaves no record;
 *   a = use_alt[i] ? alt_actions[i] : actions[i]   (the ASK bit, active_primitive_language.py:59-61);
 *   an a outside 0..5 latches CRAFT_EBADACTION, and the slot stays as it is;
 *   state = step(state, a)                          (STOP too: a no-op that keeps dir, code 5);
 *   timer -= 1; done = (a == STOP) or timer <= 0;
 *   a slot that ends freezes exactly as under craft_step: craft_step, craft_teacher and
 *   craft_reset treat it as any frozen slot.
 * Statistics go to craft_stats' counters: env-steps = slots that stepped, episodes ended = slots
 * that ended this tick, successes = those that ended with satisfies() == 1.
 * label_out (device int32[n_envs], NULL = no teacher in the launch) receives
 * DemonstrationTeacher.__call__ of the new state of every slot not frozen before the tick, a
 * slot whose episode this tick ended included (the reference keeps asking the teacher about done
 * envs, interactive_primitive_language.py:49-50, and that state no longer changes); -1 for a
 * slot frozen before the tick; -2 where the reference's teacher raises, which latches
 * CRAFT_ETEACHER only for a slot still running after the tick (the reference asks about an
 * ended env only while another env keeps its loop alive: the rollout layer decides).
 * CRAFT_EINVAL: flags != 0, use_alt without alt_actions, or (with label_out) a launch under
 * stream capture while pool rows wait for their teacher-table entries (craft_sim_sync_table).
 * Always the one-tile kernel: of craft_sim_tune_teach's knobs, lanes and table apply. */
typedef struct {
  const int32_t* actions;       /* int32[n_envs], or NULL: the hashed draw (action_seed, tick) */
  const int32_t* alt_actions;   /* int32[n_envs] or NULL */
  const uint8_t* use_alt;       /* uint8[n_envs] or NULL: nonzero -> the slot acts on alt_actions[i] */
  uint64_t action_seed;
  int64_t  tick;
  uint32_t flags;               /* must be 0: no auto-reset in this protocol */
  void*    obs;                 /* [n_envs][n_features], handle's obs format: features() of every
                                   slot's state after the tick (a frozen slot: its final state) */
  uint8_t* done;                /* 1 for a slot that is done after this tick (ended now or before) */
  int8_t*  success;             /* done slots: satisfies(own task) of the current state,
                                   1 / 0 / -1 (None); running slots: -1 */
  int32_t* action_record;       /* the action stepped, -1 for a slot done before the tick */
  int8_t*  ask_record;          /* use_alt bit of a slot that stepped, -1 otherwise */
  int8_t*  transition_code;     /* craft_transition's codes; -1 for a slot done before the tick */
  int32_t* any_live;            /* as craft_step_ex */
  int32_t* label_out;           /* NULL = no teacher in the launch */
} craft_lang_step_args_t;
int craft_step_lang(craft_sim_t* sim, const craft_lang_step_args_t* args, void* stream);

/* ---- the episode queue ---------------------------------------------------------
 * CRAFT_STEP_AUTORESET puts a finished slot back on its own spec.  The episode queue gives it
 * something new instead: a device-resident list of episode specs, a static assignment of its
 * entries to slots, and a tick (craft_step_stream) that moves a finished slot onto its next
 * entry.  One pass over a split (ImitationTrainer.evaluate, trainers/imitation.py:183-226) or an
 * endless stream of fresh episodes for a student in the loop (CRAFT_QUEUE_WRAP) both sit on it. */

/* Installs the queue: `specs` is device int32[count][5] = {scenario, x0, y0, dir0, task} (a host
 * pointer on the CPU variant), the fields and ranges craft_reset checks, 1 <= count < 2^31.  A
 * kernel checks every entry and packs it into a buffer the handle owns (8 bytes per entry:
 * scenario | task << 24, then x | y << 8 | dir << 16), so a tick never meets an invalid entry and
 * nothing is allocated on the step path.  Synchronous, like craft_pool_load.  An invalid entry
 * fails the call with CRAFT_EINVAL (the message names the first such index) and the queue
 * installed before, if any, stays in force.  Scenario indices are checked against the pool rows
 * loaded at this call; a later craft_pool_load does not invalidate the queue (its entries then
 * name whatever those rows hold).  Installing a queue does not move any slot, but the cursors of
 * a craft_episode_begin made on the previous queue mean nothing on this one: craft_step_stream
 * refuses until craft_episode_begin has been called again. */
int craft_episode_queue(craft_sim_t* sim, const int32_t* specs, int64_t count);

#define CRAFT_QUEUE_WRAP 1u   /* queue indices are taken mod count: the stream never runs out */

/* craft_reset of every slot from the queue, stream-ordered.  The slot with global id g =
 * env_id_base + i starts on entry first + g; its later episodes are first + g + k * stride,
 * k = 1, 2, ...  A caller sharding over ranks passes stride = the total envs of all ranks, and
 * every rank then runs the episodes a single large handle would have given those slots (the
 * invariant the hashed draw keeps).  With CRAFT_QUEUE_WRAP the indices are taken mod count;
 * without it an index >= count means the slot has run out, and its finished episode then freezes
 * it exactly as craft_step without auto-reset does.  The assignment is static on purpose: a
 * shared counter would balance the slots better, but which slot got which episode (and so every
 * output row) would then depend on timing.  CRAFT_EINVAL: no queue installed, stride < 1,
 * first < 0, or (without WRAP) a slot whose first index is already >= count.  `obs` as in
 * craft_reset.  A later craft_reset or craft_set_state changes a slot's state but leaves its
 * cursor alone: the slot's next restart still takes the entry after the one it was given here. */
int craft_episode_begin(craft_sim_t* sim, int64_t first, int64_t stride, uint32_t flags, void* obs,
                        void* stream);

/* craft_step_ex / craft_step_teach with CRAFT_STEP_AUTORESET, except that a slot whose episode
 * ends restarts on its next queue entry instead of its own spec.  The protocol is the same: done
 * on STOP or at the time limit, success = satisfies() of the pre-step state, no step on the
 * ending tick; done / success / reward, the action record, the transition code and the
 * statistics are craft_step_ex's.  On a restart the slot takes the entry's scenario, pose and
 * task, timer = max_timesteps, an empty inventory and nothing cleared; the init pose and the
 * spec craft_get_state reports become the entry's.  The tick's obs row and label are features()
 * and the teacher's answer of that new initial state under the new task.  A slot that has run
 * out freezes: its row is its final state and its label -1.
 *   label_out    int32[n] or NULL (no teacher in the launch), as craft_step_teach's;
 *   episode_end  int32[n]: the queue index of the episode that ended this tick, else -1;
 *   end_pose     int32[n]: x | y << 8 | dir << 16 of that episode's final state, else -1;
 *   episode_now  int32[n]: the queue index the slot runs after the tick, -1 for a frozen slot
 * (each may be NULL).  *any_live is set when some slot is still running after the tick, a slot
 * that just restarted included, so a pass over the queue has ended when it stays 0.
 * CRAFT_EINVAL: step.flags != CRAFT_STEP_AUTORESET, no craft_episode_begin since the queue was
 * installed, or (with
 * label_out) a launch under stream capture while pool rows wait for their teacher-table entries
 * (craft_sim_sync_table).  Always the one-tile kernel: of craft_sim_tune_teach's knobs, lanes and
 * table apply.  craft_step*, craft_step_lang, craft_rollout and craft_rollout_teach behave as
 * before (their auto-reset restarts a slot on the spec it has now, the queue entry it last took). */
typedef struct {
  craft_step_args_t step;
  int32_t* label_out;
  int32_t* episode_end;
  int32_t* end_pose;
  int32_t* episode_now;
} craft_stream_step_args_t;
int craft_step_stream(craft_sim_t* sim, const craft_stream_step_args_t* args, void* stream);

/* craft_step_lang on the episode queue: the language trainers' tick (step first, then the timer,
 * success read off the state the step left) whose finished slots restart on their next queue
 * entry.  It is what the three language trainers' inherited evaluate (trainers/imitation.py:
 * 183-226 over their own do_rollout) and an endless stream of fresh episodes for a language
 * student (CRAFT_QUEUE_WRAP) sit on.  Against craft_step_stream's protocol an episode that times
 * out takes max_timesteps steps, not one fewer; the ending tick moves, grabs or crafts like any
 * other; and end_pose is the pose AFTER that step.  Per slot, in this order:
 *   a slot frozen before the tick takes no step and leaves no record: action_record, ask_record
 *     and transition_code -1, done 1, success = satisfies() of its final state, label -1,
 *     episode_end, end_pose and episode_now -1;
 *   a = use_alt[i] ? alt_actions[i] : actions[i]; an a outside 0..5 latches CRAFT_EBADACTION and
 *     the slot stays as it is: no step, no timer drop, no episode end, no restart, its cursor
 *     untouched (done 0, success -1, episode_now its cursor);
 *   state = step(state, a); timer -= 1; ended = (a == STOP) or timer <= 0; the records are the
 *     action, the ask bit and the transition code of that step, on the ending tick too;
 *   ended: done 1, success = satisfies(own task) of the post-step state, episode_end = the queue
 *     index the slot was on, end_pose = x | y << 8 | dir << 16 of the post-step state, and the
 *     cursor moves on by craft_episode_begin's stride and wrap rule.
 *       A next entry exists: the slot restarts exactly as under craft_step_stream (the entry's
 *       scenario, pose and task, timer = max_timesteps, an empty inventory, nothing cleared; the
 *       init pose and the spec craft_get_state reports become the entry's).  It is running:
 *       episode_now is the new index, the obs row is features() of the new initial state, the
 *       label the teacher's answer for it under the new task (-2 latches CRAFT_ETEACHER, because
 *       the slot runs on).
 *       None: the slot freezes as under craft_step_lang; the obs row and the label are those of
 *       its final state, a -2 there does not latch, episode_now is -1.
 *   not ended: done 0, success -1, episode_end and end_pose -1, episode_now the cursor.
 * Statistics go to craft_stats as craft_step_lang counts them (stepped, ended, ended with success
 * 1).  *any_live is set when some slot is not frozen after the tick, a restarted one included.
 * CRAFT_EINVAL: step.flags != 0, use_alt without alt_actions, a misaligned obs, no
 * craft_episode_begin since the queue was installed, or with label_out the BFS-queue limit
 * (4*W*H > 1000) or a launch under stream capture while pool rows wait for their teacher-table
 * entries (craft_sim_sync_table).  Always the one-tile kernel: craft_sim_tune_teach's lanes and
 * table apply, craft_sim_tune's tile to the launch without a teacher.  craft_step*,
 * craft_step_lang and craft_step_stream behave as before; the two stream ticks share one cursor
 * per slot, so a handle may mix them. */
typedef struct {
  craft_lang_step_args_t step;   /* flags must be 0; label_out lives here */
  int32_t* episode_end;          /* as craft_step_stream */
  int32_t* end_pose;             /* pose of the final state: AFTER the ending step */
  int32_t* episode_now;
} craft_lang_stream_step_args_t;
int craft_step_lang_stream(craft_sim_t* sim, const craft_lang_stream_step_args_t* args, void* stream);

/* ---- the policy head: the student's logits chosen inside the tick ----------------
 * Between the student's last GEMM and the tick a caller otherwise runs small kernels only to turn
 * [n_envs][6] logits into int32[n_envs] actions: argmax and a cast in evaluation
 * (students/imitation.py:80), Categorical(logits).sample() in training (:82).  The entry points
 * below take the logits and choose the action themselves, by a rule written out operation by
 * operation so that both libraries (and any third implementation) give the same bits.
 *
 * The head rule.  Slot i has global id g = env_id_base + i; the tick is t; its row is the six
 * floats l[0..5] = logits[6 * i ..].  All arithmetic is IEEE binary32, round to nearest even, no
 * contraction other than the fmaf written here.
 *   1. bad = some l[k] is NaN or +inf (that is, !(l[k] < +inf)).  m = the maximum of the six, taken
 *      as m = l[0]; m = (l[k] > m) ? l[k] : m for k = 1..5.  If bad, or m == -inf, the action
 *      is -1 and nothing below runs.
 *   2. CRAFT_HEAD_ARGMAX: the action is the smallest k with l[k] == m (torch.argmax's documented
 *      choice among equal maxima).
 *   3. CRAFT_HEAD_SAMPLE:
 *        h = splitmix64(seed ^ (g << 20) ^ t)     (uint64; the mixing of craft_step's hashed draw:
 *            z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *            z = (z ^ z >> 27) * 0x94D049BB133111EB; h = z ^ z >> 31)
 *        u = (float)(h >> 40) * 2^-24             (exact: 24 bits; 0 <= u < 1)
 *        w[k] = 0 when l[k] == -inf, else craft_expf(max(l[k] - m, -80.0f))
 *        c[0] = w[0]; c[k] = c[k-1] + w[k]        (float adds, in index order)
 *        thr = u * c[5]
 *        the action is the smallest k with c[k] > thr; if there is none (thr rounded up to c[5]),
 *        the largest k with w[k] > 0.
 *      A masked action (l[k] == -inf) is never drawn: c does not rise at it.  The -80 clamp keeps
 *      every w a normal float (e^-80 = 1.8e-35), so denormal handling cannot differ anywhere.
 *   craft_expf(x), for -80 <= x <= 0:
 *        k = rintf(x * 1.44269502f)                               (0x3FB8AA3B)
 *        r = fmaf(k, -0.693145752f, x)                            (0xBF317200: ln 2, high part)
 *        r = fmaf(k, -1.42860677e-06f, r)                         (0xB5BFBE8E: ln 2, low part)
 *        p = c6; p = fmaf(p, r, c5); ... ; p = fmaf(p, r, c0)     (Horner, degree 6)
 *          c6..c0, as float bit patterns: 0x3AB566C5, 0x3C0936C6, 0x3D2AAC3F, 0x3E2AAA05,
 *          0x3EFFFFFD, 0x3F800000, 0x3F800000
 *        the result is the float whose bits are bits(p) + ((int32)k << 23)   (p in [0.70, 1.42],
 *        k >= -116: the exponent field never leaves the normal range)
 *      No library exp, no fast-math.  Within 2^-21 relative of exp(x) on [-80, 0].
 * An action of -1 is treated exactly as actions[i] = -1 is under the wrapped entry point: a
 * running slot latches CRAFT_EBADACTION (unless STOP's test or the time limit ends its episode
 * first, as for a given -1), and a slot with behavior_clone set acts on its label instead.
 * CRAFT_EINVAL for every entry point below (the message names it): a NULL head or NULL
 * head->logits, a mode other than the two, a logits base that is not 8-byte aligned. */
#define CRAFT_HEAD_ARGMAX 0
#define CRAFT_HEAD_SAMPLE 1
typedef struct {
  const float* logits;  /* device fp32 [n_envs][6], contiguous rows, base 8-byte aligned */
  int32_t mode;         /* CRAFT_HEAD_* */
  uint64_t seed;        /* SAMPLE only */
} craft_policy_head_t;

/* The head alone, one small launch: actions_out (device int32[n_envs]) = head(i) at `tick`.
 * CRAFT_EINVAL also for a NULL actions_out. */
int craft_policy_actions(craft_sim_t* sim, const craft_policy_head_t* head, int64_t tick,
                         int32_t* actions_out, void* stream);

/* craft_step_ex (label_out NULL) or craft_step_teach (label_out set) with actions[i] = head(i) at
 * step->tick, in the same single launch: the kernels read the row beside the slot's state and run
 * the head where they would draw the hashed action.  Every output, the slot state, the statistics
 * and the latched error are those of craft_policy_actions followed by the wrapped entry point on
 * its result.  CRAFT_EINVAL: the head's refusals above; step->actions != NULL (the actions are the
 * head's); then everything the wrapped entry point refuses, with its message.  Launch shapes and
 * knobs as the wrapped entry point (craft_sim_step_shape). */
int craft_step_policy(craft_sim_t* sim, const craft_step_args_t* step, const craft_policy_head_t* head,
                      int32_t* label_out, void* stream);

/* craft_step_stream likewise: args->step.actions must be NULL, actions[i] = head(i) at
 * args->step.tick.  The head's action is known before the tick decides whether the slot's episode
 * ends, so the fetch of the next queue entry is issued as early as with given actions. */
int craft_step_policy_stream(craft_sim_t* sim, const craft_stream_step_args_t* args,
                             const craft_policy_head_t* head, void* stream);

/* ---- the policy head on the language tick ------------------------------------------------------
 * The three language students decide as the imitation student does (students/
 * active_primitive_language.py:113-131, instructed_act :139-143), and the active student also asks
 * the teacher wherever entropy(softmax(l)) / ln 6 > threshold (:116-119).  In the reference the
 * instructed model's logits depend on the ask bits (an asking env's instruction is replaced before
 * instructed_act runs, trainers/active_primitive_language.py:51-57), so the order of a tick is:
 * the main model decodes; the ask bits; the instructions; the instructed model decodes; the tick.
 * craft_policy_ask is the second step as one launch; the tick takes both logit tensors and the bits.
 *
 * The ask rule.  The row l[0..5] and the arithmetic are the head rule's (binary32, round to nearest
 * even, no contraction other than the fmaf written here).  No logarithm: H = ln S - A / S > T is
 * decided as S > e^(T + A / S), with craft_expf on the side that keeps its argument in [-80, 0].
 *   1. bad and m as in step 1 of the head rule.  If bad, or m == -inf, ask = 0 and nothing below runs
 *      (the reference's NaN entropy compares false as well).
 *   2. For k = 0..5 in order: dk = max(l[k] - m, -80.0f); w[k] = 0 when l[k] == -inf, else
 *      craft_expf(dk); S = w[0], then S = S + w[k]  (S is c[5] of the head rule; craft_expf(0) is
 *      exactly 1, so S >= 1); A = 0, then A = fmaf(w[k], dk, A), skipped where l[k] == -inf
 *      (A <= 0; the entropy is ln S - A / S).
 *   3. T = threshold * LN6, LN6 = 1.79175949f (0x3FE55860, the float nearest ln 6), a rounded product;
 *      q = A / S, the correctly rounded IEEE division; x = T + q, a rounded sum (never fused with
 *      the product).
 *   4. If !(x > 0): ask = S > craft_expf(max(x, -80.0f)).
 *      Otherwise:   ask = S * craft_expf(-x) > 1.0f    (x <= ln 6: the argument is within range).
 * Against the float64 definition the three compared quantities each carry under 1e-6 absolute
 * (craft_expf's 2^-21 relative, six-term sums), so the bit can differ only where the normalised
 * entropy is within 2.5e-6 of the threshold (DESIGN.md has the measured figure).
 *
 * ask_out (device uint8[n_envs]) = the ask bit of every slot's row of head->logits; head->mode and
 * head->seed are not read.  One small launch, like craft_policy_actions.  CRAFT_EINVAL: a NULL
 * head or head->logits, a logits base that is not 8-byte aligned, a NULL ask_out, a threshold that
 * is NaN or outside [0, 1]. */
int craft_policy_ask(craft_sim_t* sim, const craft_policy_head_t* head, float threshold,
                     uint8_t* ask_out, void* stream);

/* craft_step_lang with actions[i] = head(i) at args->tick and, with alt_head, alt_actions[i] =
 * alt_head(i), in the same single launch: the slot acts on use_alt[i] ? alt_head(i) : head(i).
 * Each head has its own mode and seed (two SAMPLE heads given one seed would draw from the same
 * uniform number: seed them apart).  The kernel requests both rows and the use_alt byte beside the
 * slot's state, selects row, mode and seed per slot and runs the head once on the selection.
 * With alt_head NULL, alt_actions / use_alt may still be given as integers exactly as under
 * craft_step_lang (the interactive trainer, where every env follows the instructed model, is
 * simply head = the instructed logits).  Every output, the slot state, the statistics and the
 * latched error are those of craft_policy_actions on each head followed by craft_step_lang on the
 * two vectors: only the selected head's -1 can latch CRAFT_EBADACTION, a bad main row on a slot
 * that takes its alt action is harmless, as an integer actions[i] = -1 is there.
 * CRAFT_EINVAL (the message names the reason): the head's refusals, for head and then for
 * alt_head; args->actions != NULL; alt_head together with alt_actions != NULL; alt_head without
 * use_alt; then everything craft_step_lang refuses, with its message. */
int craft_step_lang_policy(craft_sim_t* sim, const craft_lang_step_args_t* args,
                           const craft_policy_head_t* head, const craft_policy_head_t* alt_head,
                           void* stream);

/* craft_step_lang_stream likewise (args->step is the craft_lang_step_args_t the rules above read). */
int craft_step_lang_policy_stream(craft_sim_t* sim, const craft_lang_stream_step_args_t* args,
                                  const craft_policy_head_t* head, const craft_policy_head_t* alt_head,
                                  void* stream);

/* n_ticks consecutive craft_step ticks (tick0, tick0+1, ...) in one launch, with
 * results identical to n_ticks craft_step calls: each workgroup keeps its envs
 * on chip between ticks, so the per-tick prologue overlaps other workgroups'
 * observation stores.  For rollouts whose actions do not depend on the
 * observations: `actions` is device int32[n_ticks][n_envs] or NULL for the
 * hashed draw.  Tick t writes ring slot t % ring of each output: obs
 * [ring][n_envs][n_features] (obs format; each slot 16-byte aligned), reward /
 * done / success [ring][n_envs]; each may be NULL.
 * Ordering: one handle's craft_rollout launches must run in issue order, i.e. on one stream (or
 * streams the caller orders): the work-unit counter they share is advanced by each launch, not
 * re-zeroed.  A launch captured into a HIP graph (hipStreamIsCapturing) uses a separate counter
 * that a memset captured with it zeroes, so a graph may be replayed any number of times, in
 * order with each other and with eager launches.  Every captured launch of one handle shares
 * that one counter: two captured graphs, or one graph replayed on two streams, must never run
 * concurrently (unsupported: their work units would be skipped or repeated, undetected). */
int craft_rollout(craft_sim_t* sim, const int32_t* actions, uint64_t action_seed, int64_t tick0,
                  int32_t n_ticks, uint32_t flags, void* obs, int32_t ring, float* reward,
                  uint8_t* done, int8_t* success, void* stream);

/* craft_rollout on the episode queue: n_ticks consecutive craft_step_stream ticks (tick0,
 * tick0 + 1, ...; label_out NULL) in one launch, with results identical to those n_ticks calls
 * with the same actions: every output row of every tick, each slot's state, inventory, cleared
 * cells, init pose and spec as craft_get_state reports them, its queue cursor, the craft_stats
 * counters and the latched error.  A slot whose episode ends restarts on its next queue entry in
 * the middle of the launch, any number of times.  For rollouts over many scenarios whose actions
 * do not depend on the observations: the hashed draw, or recorded action sequences replayed into
 * observations (Python: rollout.replay).  `actions` is device int32[n_ticks][n_envs] or NULL for
 * the hashed draw; tick t writes ring slot t % ring of every output (each may be NULL); n_ticks
 * == 0 is a no-op.  The cursor is the one craft_step_stream and craft_step_lang_stream move, so a
 * handle may mix the three between launches.
 * CRAFT_EINVAL: flags != CRAFT_STEP_AUTORESET, no craft_episode_begin since the queue was
 * installed, n_ticks < 0, ring < 1, tick0 < 0, or an obs ring slot that is not 16-byte aligned.
 * Launch shape: always the split-producer kernel on 512 threads, one work unit per tile for the
 * whole launch, on 32-env tiles; 16-env tiles where craft_sim_tune chose 16 or where two staged
 * observation buffers of 32 envs do not fit a workgroup's LDS.  craft_sim_tune_rollout's chunk
 * and threads knobs do not apply; craft_sim_tune's store policy does.  Ordering and graph capture
 * as craft_rollout: the launches share its work-unit counter (one stream, or streams the caller
 * orders), a captured launch uses the graph's own counter and the memset captured with it, and
 * nothing is allocated on the step path. */
typedef struct {
  const int32_t* actions;   /* int32[n_ticks][n_envs], or NULL: the hashed draw */
  uint64_t action_seed;
  int64_t  tick0;
  int32_t  n_ticks;
  uint32_t flags;           /* must be CRAFT_STEP_AUTORESET */
  int32_t  ring;            /* ring slots of every output (>= 1); tick t writes slot t % ring */
  void*    obs;             /* [ring][n_envs][n_features], obs format, each slot 16-byte aligned */
  float*   reward;          /* [ring][n_envs] */
  uint8_t* done;
  int8_t*  success;
  int32_t* episode_end;     /* [ring][n_envs], as craft_step_stream's */
  int32_t* end_pose;
  int32_t* episode_now;
} craft_rollout_stream_args_t;
int craft_rollout_stream(craft_sim_t* sim, const craft_rollout_stream_args_t* args, void* stream);

/* Installs recorded action sequences for the installed queue, one per entry: `actions` is device
 * int32[count][max_timesteps] (host on the CPU variant), row e = entry e's actions then -1 up to
 * max_timesteps: the layout of craft_episode_summary's actions_out.  count must equal the queue's
 * length.  A row is valid when it is 1..max_timesteps values in 0..5 followed only by -1, and
 * either its last action is its only STOP or it is max_timesteps long.  A kernel checks every row
 * and packs it into a buffer the handle owns (one byte per action, rows of max_timesteps rounded
 * up to 4 bytes, padded with STOP); synchronous, like craft_episode_queue.  An invalid row fails
 * the call with CRAFT_EINVAL (the message names the first such entry) and the tape installed
 * before, if any, stays in force; so it does when the buffer cannot be allocated (CRAFT_ENOMEM).
 * actions == NULL with count == 0 drops the tape.  craft_episode_queue drops it too (its rows
 * mean nothing on another queue).  Moves no slot and no cursor; needs no craft_episode_begin.
 * CRAFT_EINVAL, tested in this order: no queue installed; actions NULL with count != 0, or count
 * != the queue's length; an invalid row. */
int craft_episode_actions(craft_sim_t* sim, const int32_t* actions, int64_t count);

/* craft_rollout_stream whose actions are the installed tape's (craft_episode_actions): n_ticks
 * consecutive craft_step_stream ticks (label_out NULL) in one launch, exactly as
 * craft_rollout_stream runs them, where tick k's action for slot i is read on the device.  With
 * c the slot's queue cursor and p = max_timesteps - timer, both taken before the tick: for
 * 0 <= p < max_timesteps the action is tape[c][p], and -1 padding reads as STOP; for any other p
 * (which only craft_set_state can bring about, with a timer of 0 or above max_timesteps) it is
 * STOP, and nothing latches for it.  A frozen slot's action is unused.  Every ring row, slot
 * state, cursor, craft_stats counter and latched error is identical to those n_ticks
 * craft_step_stream calls with those actions, and so to craft_rollout_stream given the same
 * [n_ticks][n_envs] tensor.  Under the imitation protocol an episode then takes exactly as many
 * ticks as its row has actions: a replay pass (Python: rollout.replay) needs no host work per
 * tick, can be captured into a graph with no actions buffer to refresh, and runs epochs under
 * CRAFT_QUEUE_WRAP.
 * Two more outputs, [ring][n_envs] each and each may be NULL, both of the slot after the tick
 * (a slot that restarted on this tick included): step_now is -1 for a frozen slot, else
 * max_timesteps - timer, the number of actions of the current episode already taken (0 right
 * after a restart); action_next is -1 for a frozen slot, else the action the rule above gives
 * for the next tick.  With episode_now they are the (episode, step, action) of the state the
 * tick's observation row shows.
 * The action depends only on (cursor, timer), so nothing is carried between launches: a handle
 * may mix this entry point with the four other stream entry points, craft_set_state and
 * craft_reset between launches.  n_ticks == 0 is a no-op.
 * CRAFT_EINVAL, tested in this order: everything craft_rollout_stream refuses, in its order;
 * roll.actions != NULL; no tape installed for the current queue.
 * Launch shape, ring rule, ordering, the work-unit counter shared with craft_rollout, graph
 * capture (the graph's own counter and the memset captured with it) and "nothing allocated on
 * the step path" as craft_rollout_stream; craft_sim_tune's tile and store policy apply.
 * Measured against craft_rollout_stream with given actions: DESIGN.md "Recorded actions on the
 * queue". */
typedef struct {
  craft_rollout_stream_args_t roll;  /* roll.actions must be NULL; action_seed is ignored */
  int32_t* step_now;     /* [ring][n_envs] or NULL */
  int32_t* action_next;  /* [ring][n_envs] or NULL */
} craft_rollout_replay_args_t;
int craft_rollout_replay(craft_sim_t* sim, const craft_rollout_replay_args_t* args, void* stream);

/* craft_rollout with the DemonstrationTeacher in the same launch: n_ticks ticks, and after each
 * one DemonstrationTeacher.__call__ (teachers/demonstration.py:9-30) of every slot's new state,
 * as n_ticks craft_step_teach calls would give, with each tick's action taken per slot from
 *   - its label (the teacher's action for its current state): every slot when label_actions
 *     (make_data.get_reference_actions, make_data.py:146-152: the demonstrations), or the slots
 *     with behavior_clone[i] set (DAgger's mix, trainers/imitation.py:47-57);
 *   - otherwise the policy: actions[k][i] (device int32[n_ticks][n_envs]) or the hashed draw.
 * The label of a slot's state before tick0 comes from label_in (device int32[n_envs]: craft_teacher's
 * answer, or the last labels ring slot of the previous launch); required when labels feed actions.
 * Tick k = tick0 + k writes ring slot k % ring of each output (each may be NULL): obs
 * [ring][n_envs][n_features] (obs format), reward / done / success as craft_rollout, labels
 * int32 [ring][n_envs] (the label of the slot's state after the tick: -1 for a slot the tick left
 * frozen, -2 and CRAFT_ETEACHER latched where the reference raises), action_record int32
 * [ring][n_envs] (the action taken, -1 for a slot already done: action_seqs).  Episode statistics
 * accumulate as for craft_step.  Ordering as craft_rollout (one stream; a captured launch uses the
 * graph's own counter).  Replaces the per-tick loop of trainers/imitation.py:43-73 with the
 * teacher queried every tick, and make_data.get_reference_actions. */
typedef struct {
  const int32_t* actions;          /* int32[n_ticks][n_envs] policy actions, or NULL: the hashed draw */
  const uint8_t* behavior_clone;   /* uint8[n_envs] 0/1: the slot acts on its label, or NULL */
  int32_t label_actions;           /* 1: every slot acts on its label */
  const int32_t* label_in;         /* int32[n_envs] labels of the states before tick0 */
  uint64_t action_seed;
  int64_t tick0;
  int32_t n_ticks;
  uint32_t flags;                  /* CRAFT_STEP_AUTORESET */
  int32_t ring;                    /* ring slots of every output (>= 1) */
  void* obs;
  float* reward;
  uint8_t* done;
  int8_t* success;
  int32_t* labels;
  int32_t* action_record;
} craft_rollout_teach_args_t;
int craft_rollout_teach(craft_sim_t* sim, const craft_rollout_teach_args_t* args, void* stream);

/* craft_rollout_teach on the episode queue: n_ticks consecutive craft_step_stream ticks (tick0,
 * tick0 + 1, ...; label_out set) in one launch.  Tick k of that loop gets
 *   step.actions        = actions[k], or NULL for the hashed draw;
 *   step.ref_actions    = the labels the tick before produced (label_in for k = 0);
 *   step.behavior_clone = behavior_clone, or all ones when label_actions, or NULL when labels
 *                         feed no actions (neither is set),
 * and the results are identical to those n_ticks calls: every ring row of every tick (obs in
 * every format, reward, done, success, labels, action_record, episode_end, end_pose,
 * episode_now), each slot's state, inventory, cleared cells, init pose and spec as
 * craft_get_state reports them, its queue cursor, the craft_stats counters and the latched
 * error.  A slot whose episode ends restarts on its next queue entry in the middle of the launch,
 * any number of times.  The tick's label for a restarted slot is the teacher's answer for the new
 * initial state under the new task, and that label is what the slot acts on next tick when it
 * acts on labels; a slot that has run out freezes, with label -1.  It is what demonstration
 * generation over a whole split (make_data.get_reference_actions, make_data.py:146-152,188-216;
 * Python: rollout.demonstrations) and DAgger over fresh episodes (trainers/imitation.py:43-73 with
 * CRAFT_QUEUE_WRAP) sit on.  The cursor is the one craft_step_stream, craft_step_lang_stream and
 * craft_rollout_stream move, so a handle may mix all four between launches.  n_ticks == 0 is a
 * no-op.
 * CRAFT_EINVAL, tested in this order: teach.flags != CRAFT_STEP_AUTORESET; n_ticks < 0, ring < 1
 * or tick0 < 0; the BFS-queue limit (4*W*H > 1000); label_actions or behavior_clone without
 * label_in; an obs ring slot that is not 16-byte aligned; no craft_episode_begin since the queue
 * was installed; and (the HIP library) a launch under stream capture while pool rows wait for
 * their teacher-table entries (craft_sim_sync_table before capturing right after a pool load).
 * Launch shape as craft_rollout_teach: 512 threads, one work unit per tile (32 envs at 3x3
 * windows, 16 at wider ones) for the whole launch; craft_sim_tune_teach's table knob applies,
 * observation stores are nontemporal unless craft_sim_tune set a policy.  Ordering and graph
 * capture as craft_rollout_teach: the launches share craft_rollout's work-unit counter (one
 * stream, or streams the caller orders), a captured launch uses the graph's own counter and the
 * memset captured with it, and nothing is allocated on the step path.
 * Measured against the per-tick craft_step_stream(label_out) loop and craft_rollout_teach:
 * DESIGN.md "The teacher K-tick launch on the queue". */
typedef struct {
  craft_rollout_teach_args_t teach;  /* flags must be CRAFT_STEP_AUTORESET */
  int32_t* episode_end;              /* [ring][n_envs], as craft_step_stream's */
  int32_t* end_pose;
  int32_t* episode_now;
} craft_rollout_teach_stream_args_t;
int craft_rollout_teach_stream(craft_sim_t* sim, const craft_rollout_teach_stream_args_t* args, void* stream);

/* The per-episode results of a queue pass: turns the per-tick records of craft_step_stream,
 * craft_step_lang_stream, craft_rollout_stream or craft_rollout_teach_stream ([ticks][n_envs]
 * rows in tick order, as those entry points write them) into results indexed by queue entry,
 * what ImitationTrainer.evaluate and the training log report (trainers/imitation.py:79-91,
 * 183-226).  Reads the installed queue, the pool and the teacher table; touches no slot state
 * (state, inventory, cleared cells, cursors, statistics) and does not need craft_episode_begin.
 * Per slot i, in tick order, with a running count that starts at run[i] (0 without run): for
 * every tick t with e = episode_end[t][i] >= 0 the slot's episode ends.  e >= count (the padding
 * of a short split) is skipped; e >= the queue's length is skipped and latches CRAFT_ERANGE with
 * the slot, as does any episode_end value < -1 (which is no end).  Otherwise
 *   length_out[e]   = ticks since the slot's previous end, or since the episode began run[i]
 *                     ticks before row 0, the ending tick included;
 *   success_out[e]  = success[t][i]; flags_out[0] = 1 when that is < 0 (imitation.py:68);
 *   end_pose_out[e] = end_pose[t][i];
 *   actions_out[e]  = the action_record entries of exactly those ticks (at positions run[i] + k
 *                     for an episode that began before row 0: the calls before wrote the earlier
 *                     ones), then -1 up to max_timesteps; positions >= max_timesteps are dropped
 *                     while length_out keeps the true count;
 *   distance_out[e] = what craft_rollout_distances documents for (the entry's task, that
 *                     success, that pose) on the entry's pool row with nothing cleared: -1 for
 *                     goals other than `get`, 0 for a get that did not fail, else the path
 *                     length; -1 where find_closest_resources returns None (the grid holds no
 *                     target, or none of them can be reached) and -2 where it raises (an
 *                     unreachable target after a reachable one, base.py:31), both setting
 *                     flags_out[1] and latching nothing; a pose outside the interior latches
 *                     CRAFT_EINVAL with the slot and gives -2.
 * After the last row, with run: run[i] = the ticks of the still-running episode, 0 for a slot
 * that has run out (episode_now[i] < 0, where episode_now is given); with run and actions_out the
 * running episode's actions so far are written at their positions in row episode_now[i] when that
 * is in [0, count), and the call over the next launch's records completes the row.
 * Entries for which the records hold no end are left untouched: the caller pre-fills them.  With
 * CRAFT_QUEUE_WRAP an entry may end more than once within one call; its outputs are then those
 * of one of the ends, unspecified which (the HIP library: each output array holds one end's
 * value, and distance_out is the distance of the success_out and end_pose_out it left).
 * flags_out is only ever set to 1, by plain stores, and never zeroed here.  ticks == 0 is a
 * no-op.  Stream-ordered; allocates nothing.
 * CRAFT_EINVAL, tested in this order, before any work: args NULL; a NULL episode_end, end_pose,
 * success, length_out, success_out, end_pose_out or flags_out; ticks < 0; no queue installed;
 * count outside 1 .. the queue's length; actions_out without action_record; run with
 * action_record but without episode_now; with distance_out, the BFS-queue limit (4*W*H > 1000);
 * and (the HIP library, with distance_out) a launch under stream capture while pool rows wait for
 * their teacher-table entries (craft_sim_sync_table first).
 * Two launches in the HIP library: one lane per slot scans its record column; then, with
 * distance_out, lane pairs or quads per queue entry run the BFS of the failed get episodes the
 * teacher table did not answer (DESIGN.md "The per-episode summary of a queue pass"). */
typedef struct {
  const int32_t* episode_end;    /* device int32[ticks][n_envs], as the stream entry points write it */
  const int32_t* end_pose;       /* int32[ticks][n_envs] */
  const int8_t*  success;        /* int8 [ticks][n_envs] */
  const int32_t* action_record;  /* int32[ticks][n_envs], or NULL */
  int32_t  ticks;                /* rows of the records; 0 is a no-op */
  int32_t* run;                  /* int32[n_envs] in/out, or NULL (= all zero, nothing written back):
                                    ticks each slot's current episode had already run before row 0 */
  const int32_t* episode_now;    /* int32[n_envs]: the episode_now row of the records' LAST tick;
                                    required when run and action_record are both set */
  int64_t  count;                /* outputs cover queue entries [0, count), 1 <= count <= queue length */
  int32_t* length_out;           /* int32[count]: ticks the episode ran, its ending tick included */
  int8_t*  success_out;          /* int8 [count] */
  int32_t* end_pose_out;         /* int32[count]: the x | y << 8 | dir << 16 word */
  int32_t* distance_out;         /* int32[count], or NULL: no BFS runs */
  int32_t* actions_out;          /* int32[count][max_timesteps], or NULL; needs action_record */
  int32_t* flags_out;            /* int32[2], only ever set to 1 by plain stores, never zeroed here */
} craft_episode_summary_args_t;
int craft_episode_summary(craft_sim_t* sim, const craft_episode_summary_args_t* args, void* stream);

/* Sums the episode statistics accumulated by craft_step into stats_out
 * (device int64[3] = {successes, episodes ended, env-steps}) — the scalar
 * summary a multi-GPU run all-reduces over RCCL.  reset != 0 zeroes the
 * partial sums afterwards. */
int craft_stats(craft_sim_t* sim, int64_t* stats_out, int32_t reset, void* stream);

/* ---- reference-granular surface (CraftState methods), over slot lists ----
 * For every call below, n == 0 is a no-op that returns CRAFT_OK (pointers unused). */

/* CraftState.step (craft.py:332-424) as a pure transition: slot dst[i] becomes
 * step(slot src[i], actions[i]) — src == dst updates in place, src != dst keeps
 * the old state (the reference's states are immutable).  actions[i] < 0 is a
 * no-op copy.  src/dst NULL = identity over n slots.  Device int32 arrays.
 * code_out (int8[n], may be NULL) receives what PrimitiveLanguageTeacher.describe
 * reads off the (state, next state) pair (teachers/primitive_language.py:61-85):
 * 0..3 = moved by the coord_change of DOWN/UP/LEFT/RIGHT, 4 = did not move and
 * the inventory changed, 5 = neither, -1 = no step (action < 0). */
int craft_transition(craft_sim_t* sim, const int32_t* src, const int32_t* dst,
                     const int32_t* actions, int64_t n, int8_t* code_out, void* stream);

/* CraftState.features() (craft.py:296-330) and satisfies() (craft.py:285-294)
 * for n slots (NULL = identity).  obs: [n][n_features] (obs format) or NULL; sat: int8[n]
 * (-1 = None, 0/1) for task tasks[i] (NULL = the slot's own task) or NULL. */
int craft_observe(craft_sim_t* sim, const int32_t* slots, int64_t n, const int32_t* tasks,
                  void* obs, int8_t* sat, void* stream);

/* The per-env part of the rollout's summary (trainers/imitation.py:79-91), one launch over
 * every slot after a do_rollout: tasks int32[n] (each slot's task), success int8[n]
 * (1 / 0 / -1 for None), action_seqs int32[ticks][n] (the action record, -1 where the env did
 * not act).  Per slot: is_get_out = the task's goal is `get`; distances_out = -1 for other
 * goals, 0 for a success, else len(find_closest_resources(task.arg)) on world.init_state(
 * grid, pos, dir): the slot's initial grid (its pool row, nothing cleared) at its current pose
 * (-1 where the grid holds no target, -2 where a target is unreachable: base.py:31); n_actions_out
 * = the action record's non-negative entries (len(action_seqs[i])).  flags_out int32[2] (zeroed
 * here): [0] some success is None (imitation.py:68 asserts), [1] a failed get task has no
 * reachable target, in either case (the reference raises one TypeError, len(None), at
 * imitation.py:88-89 or base.py:31).  The env states are not modified.
 * Replaces trainers/imitation.py:79-91's per-env loop. */
int craft_rollout_distances(craft_sim_t* sim, const int32_t* tasks, const int8_t* success,
                            const int32_t* action_seqs, int32_t ticks, int32_t* distances_out,
                            uint8_t* is_get_out, int32_t* n_actions_out, int32_t* flags_out,
                            void* stream);

/* DemonstrationTeacher.__call__ (teachers/demonstration.py:9-30) for n slots:
 * find_incomplete_subtask over the hint tree then the BFS of
 * find_closest_resources/shortest_path (teachers/base.py:10-87).
 * action_out int32[n]; path_len_out int32[n] (may be NULL) receives
 * len(best_action_seq) of find_closest_resources for the task's own goal_arg
 * (the trainer's `distances`, trainers/imitation.py:79-91), -1 if no target.
 * Where the reference raises (base.py:24 assert, base.py:31 len(None),
 * demonstration.py:18 assert) the item gets -2 and CRAFT_ETEACHER latches.
 * slots[i] == -1 skips item i, and a frozen slot (an episode craft_step ended
 * without auto-reset) yields action -1 (path length -1, no error): the
 * trainer's ref_actions[i] = -1 for a done env (trainers/imitation.py:50-51). */
int craft_teacher(craft_sim_t* sim, const int32_t* slots, int64_t n, const int32_t* tasks,
                  int32_t* action_out, int32_t* path_len_out, void* stream);

/* State I/O for the Python CraftState shim and for parity tests (device
 * arrays, n slots, NULL slot list = identity).  grid: uint8[n][W*H] current
 * kind ids; inventory: int32[n][n_kinds]; agent: int32[n][4] = {x, y, dir, timer};
 * spec: int32[n][5] = {scenario, x0, y0, dir0, task}. */
int craft_get_state(craft_sim_t* sim, const int32_t* slots, int64_t n, int32_t* agent,
                    int32_t* inventory, uint8_t* grid, int32_t* spec, void* stream);
/* Sets slots to (scenario grid with no removals, agent, inventory); spec as above. */
int craft_set_state(craft_sim_t* sim, const int32_t* slots, int64_t n, const int32_t* spec,
                    const int32_t* agent, const int32_t* inventory, void* stream);

/* make_data.sample_scenario (make_data.py:105-144) on the GPU, straight into pool
 * rows [first, first + count): boundary ring, n_per_primitive of each primitive,
 * then the workshops, each placed by random_free with its connectivity checks,
 * then the initial position (init_pos_out: device int32[count][2], may be NULL).
 * Scenario s draws from its own splitmix64 stream keyed by seed and its global
 * id scenario_id0 + s (numpy's sequential MT19937 stream cannot be split across
 * lanes), so results do not depend on how ids are sharded; otherwise the
 * algorithm and acceptance tests are make_data.py's.  No de-duplication.  Where
 * a placement finds no valid cell in 2^20 draws, CRAFT_EINVARIANT latches. */
int craft_pool_generate(craft_sim_t* sim, uint64_t seed, int64_t scenario_id0, int32_t first,
                        int32_t count, int32_t boundary_kind, const int32_t* primitives,
                        int32_t n_primitive_kinds, int32_t n_per_primitive,
                        const int32_t* workshop_kind, int32_t n_workshops, int32_t* init_pos_out,
                        void* stream);

/* ---- host-side scenario generation ------------------------------------------ */

/* make_data.sample_scenario (make_data.py:105-144) with `random_free`
 * (make_data.py:74-103) and `all_free_cells_reachable` (make_data.py:27-72),
 * drawing from numpy's legacy RandomState(seed) MT19937 stream bit-exactly.
 * Generates `count` scenarios (each rejected and redrawn while it duplicates an
 * earlier one when `dedup`, make_data.py:167-177).  grids_out: host
 * uint8[count][W*H]; init_pos_out: host int32[count][2].  `primitives` lists the
 * primitive kind ids in the iteration order of cookbook.primitives with gold/gem
 * already removed (make_data.py:128-134); workshops are kinds workshop_kind[0..n_ws).
 * The MT19937 state after the last draw is written to mt_state_out (625 uint32,
 * may be NULL) so a caller can continue numpy's stream. */
int craft_sample_scenarios(int32_t width, int32_t height, int32_t boundary_kind,
                           const int32_t* primitives, int32_t n_primitive_kinds,
                           int32_t n_per_primitive, const int32_t* workshop_kind,
                           int32_t n_workshops, uint32_t seed, int32_t count, int32_t dedup,
                           uint8_t* grids_out, int32_t* init_pos_out, uint32_t* mt_state_out);

#ifdef __cplusplus
}
#endif
#endif /* PSKETCH_CRAFT_H */
