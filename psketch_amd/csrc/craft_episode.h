// craft_episode.h — the one definition of what every tick kernel must agree on: the per-env
// body of ImitationTrainer.do_rollout (trainers/imitation.py:59-73) in pieces, the language
// trainers' variant of it (tile_kernel's MODE_LANG), the episode queue's restart (MODE_STREAM,
// MODE_LANG_STREAM),
// and the K-tick kernels' cleared-cell bookkeeping.
//
// Everything here is __device__ __forceinline__, works on state passed by reference, touches
// no LDS of its own and has no barrier, so a kernel keeps its own scheduling (wave roles,
// parity buffers, staging, stamp hooks between the pieces) and only the arithmetic is shared.
// Used by tile_kernel, tick2_kernel (one tick per launch: the episode's cleared cells are the
// 256-bit mask in registers) and by rollout_kernel, rollout_split_kernel and
// rollout_teach_kernel (K ticks per launch: the LDS grid row is the record, and a ClearList
// remembers which of its cells an auto-reset has to restore).  The CPU variant
// (craft_cpu.cpp) keeps its own copies on purpose: it is the second implementation these are
// checked against.
#pragma once
#include "craft_device.h"

namespace craft {

// ---- the tick's action and the protocol step --------------------------------------------------

// The policy's stand-in: a uniform draw over the 6 actions, a pure function of (seed, global env
// id, tick), so that any kernel (and the CPU variant) replays the same rollout.
__device__ __forceinline__ int hashed_action(const SimView& v, uint64_t seed, int64_t slot, int64_t tick) {
  const uint64_t gid = (uint64_t)(v.env_base + slot);
  return (int)((uint32_t)(splitmix64(seed ^ (gid << 20) ^ (uint64_t)tick) >> 32) % 6u);
}

// False for a slot that reset / set_state never initialised (the caller latches CRAFT_EINVAL).
__device__ __forceinline__ bool state_in_range(const SimView& v, const Agent& s) {
  return !(s.x < 1 || s.x > v.W - 2 || s.y < 1 || s.y > v.H - 2 || s.scen >= v.pool_count);
}

// imitation.py:59-73: a frozen env is done and not counted; a running one spends a timestep and
// ends on STOP or at the time limit, restarting in place under CRAFT_STEP_AUTORESET.
// (flags by reference: a kernel-argument word is then loaded where it is used, as when the
// step was written out in the kernel, and the scalar registers come out the same)
__device__ __forceinline__ void protocol_step(Agent& s, const int& act, const uint32_t& flags, int& d, int& counted, bool& restart) {
  if (s.frozen) {
    d = 1;
  } else {
    counted = 1;
    s.timer -= 1;
    d = (act == CRAFT_STOP) || s.timer <= 0;
    restart = d && (flags & CRAFT_STEP_AUTORESET);
  }
}

// The language trainers' tick (trainers/primitive_language.py:45-66, interactive_primitive_
// language.py:43-76, active_primitive_language.py:44-87; craft_step_lang), in two pieces around
// the caller's CraftState.step.  Before it: a frozen env is done and leaves no record; a running
// one steps whatever its action (STOP too), unless the action is none of the six (bad: the
// caller latches CRAFT_EBADACTION and the slot stays as it is).
__device__ __forceinline__ void language_step_begin(const Agent& s, const int& act, int& d, int& counted, bool& bad) {
  if (s.frozen) {
    d = 1;
  } else {
    bad = act < 0 || act >= CRAFT_N_ACTIONS;
    counted = !bad;
  }
}
// After it: only now the timer drops and done latches (the env freezes as under craft_step);
// the caller reads satisfies() off the state the step left.
__device__ __forceinline__ void language_step_end(Agent& s, const int& act, int& d) {
  s.timer -= 1;
  d = (act == CRAFT_STOP) || s.timer <= 0;
  if (d) {
    s.frozen = 1;
    s.timer = max(s.timer, 0);
  }
}

// CraftScenario.init (craft.py:268-273) of the agent; the caller empties the inventory and
// restores the grid (a mask clear, or ClearList::restore).
__device__ __forceinline__ void restart_agent(Agent& s, uint32_t init_word, int maxT) {
  s.x = init_word & 0xff; s.y = (init_word >> 8) & 0xff; s.dir = (init_word >> 16) & 3;
  s.timer = maxT;
}

// ---- the episode queue (craft_step_stream: tile_kernel's MODE_STREAM) -------------------------
// A slot's cursor is the queue index of the episode it runs, -1 once it has run out.  Its next
// episode is `step` entries on: under wrap step = stride mod count and the index wraps, else
// step = min(stride, count) and an index past the end means there is none (-1).  count < 2^31
// and cur < count (craft_episode_queue / craft_episode_begin see to it), so the sum fits 32 bits.
__device__ __forceinline__ int32_t queue_next(int32_t cur, const uint32_t& count, const uint32_t& step, const uint32_t& wrap) {
  if (cur < 0) return -1;
  uint32_t nx = (uint32_t)cur + step;
  if (nx >= count) {
    if (!wrap) return -1;
    nx -= count;
  }
  return (int32_t)nx;
}

// Whether protocol_step will end the slot's episode this tick: known from the state word and the
// action alone, so the next queue entry can be fetched beside the scenario row.
__device__ __forceinline__ bool episode_ends(const Agent& s, int act) {
  return !s.frozen && (act == CRAFT_STOP || s.timer <= 1);
}

// The same for the language tick (craft_step_lang_stream): language_step_begin and
// language_step_end will step and end the episode, so an action that is none of the six ends
// nothing.
__device__ __forceinline__ bool language_episode_ends(const Agent& s, int act) {
  return !s.frozen && act >= 0 && act < CRAFT_N_ACTIONS && (act == CRAFT_STOP || s.timer <= 1);
}

// A packed queue entry (.x = scenario | task << 24, .y = the init word) as the agent's new
// episode; the caller empties the inventory and the mask and reloads the grid row.
__device__ __forceinline__ void restart_from_entry(Agent& s, const uint2& e, int maxT) {
  s.scen = (int)(e.x & 0xffffffu);
  s.task = (int)(e.x >> 24);
  restart_agent(s, e.y, maxT);
}

// x | y << 8 | dir << 16: an init word, and craft_step_stream's end_pose.
__device__ __forceinline__ uint32_t pose_word(const Agent& s) {
  return (uint32_t)s.x | ((uint32_t)s.y << 8) | ((uint32_t)s.dir << 16);
}

// craft_rollout_replay's action of a slot on queue entry `cur` in state s: byte p = maxT - timer of
// the entry's tape row (one byte per action, rows of `stride` >= maxT bytes padded with STOP, as
// craft_episode_actions packs them), STOP for a p outside the episode (a timer craft_set_state put
// at 0 or above maxT).  A slot without an entry reads nothing; its action is unused.
__device__ __forceinline__ int tape_action(const uint8_t* tape, const int& stride, int32_t cur, const Agent& s,
                                           const int& maxT) {
  const int p = maxT - s.timer;
  if (cur < 0 || p < 0 || p >= maxT) return CRAFT_STOP;
  return (int)tape[(int64_t)cur * stride + p];
}

// pool[scenario] (L2-resident) into the env's LDS grid row, in the lanes that restart onto another
// scenario only: every 16-byte chunk of a batch of QB is requested before the first is used, so
// the restart costs one more L2 round trip per batch (QB 16: the whole row at once).
template <int QB>
__device__ __forceinline__ void reload_grid_row(const uint4* pool_row, uint32_t* grid, const int& CS) {
  const int nchunk = CS >> 4;
#pragma unroll
  for (int b = 0; b < CRAFT_MAX_CELLS / 16; b += QB) {
    uint4 c[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q)
      if (b + q < nchunk) c[q] = pool_row[b + q];
#pragma unroll
    for (int q = 0; q < QB; ++q)
      if (b + q < nchunk) {
        grid[4 * (b + q) + 0] = c[q].x; grid[4 * (b + q) + 1] = c[q].y;
        grid[4 * (b + q) + 2] = c[q].z; grid[4 * (b + q) + 3] = c[q].w;
      }
  }
}

// An episode that ends without auto-reset stays as it is until the next reset.
__device__ __forceinline__ void freeze_agent(Agent& s) {
  s.frozen = 1;
  s.timer = max(s.timer, 0);
}

// The cell the agent faces (what USE acts on), x-major.
__device__ __forceinline__ int facing_cell(const Agent& s, int H) {
  return (s.x + dir_dx(s.dir)) * H + (s.y + dir_dy(s.dir));
}

// satisfies() of the pre-step state where the grid row is still pool[scenario] and this
// episode's clears are the mask m (the one-tick kernels): a cleared facing cell reads 0.
__device__ __forceinline__ int satisfies_masked(const SimView& v, const uint8_t* g, const uint8_t* iv,
                                                const uint32_t (&m)[8], const Agent& s, uint32_t tt) {
  const int fc = facing_cell(s, v.H);
  uint32_t mw = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) mw |= (w == (fc >> 5)) ? m[w] : 0u;
  return satisfies_with(
      tt, [&](int arg) __attribute__((always_inline)) { return (int)iv[arg]; },
      [&]() __attribute__((always_inline)) { return ((mw >> (fc & 31)) & 1u) ? 0 : (int)g[fc]; });
}

// x | y << 8 | dir << 16 | 1 << 24, or 0 for a slot the tick could not run: what the scatter
// (and the teacher) read of the agent.
__device__ __forceinline__ uint32_t agent_word(const Agent& s, bool live) {
  return live ? ((uint32_t)s.x | ((uint32_t)s.y << 8) | ((uint32_t)s.dir << 16) | (1u << 24)) : 0u;
}

// ---- the tick's outputs -----------------------------------------------------------------------

// imitation.py:68-70: reward 1 for an episode that ends, this tick, with its task satisfied.
__device__ __forceinline__ bool rewarded(const int& counted, const int& d, const int& succ) { return counted && d && succ == 1; }

// a: TileArgs or RolloutArgs (their done / sat / reward arrays, each optional), o: the index.
template <class Args>
__device__ __forceinline__ void store_outputs(const Args& a, int64_t o, const int& d, const int& succ, const int& counted) {
  if (a.done) a.done[o] = (uint8_t)d;
  if (a.sat) a.sat[o] = (int8_t)succ;
  if (a.reward) a.reward[o] = rewarded(counted, d, succ) ? 1.0f : 0.0f;
}

// The same three as one LDS word for a wave that stores them later: done | success << 8 |
// reward << 16 | 1 << 24 (0: nothing to store).
__device__ __forceinline__ uint32_t pack_outputs(const int& d, const int& succ, const int& counted) {
  return (uint32_t)(uint8_t)d | ((uint32_t)(uint8_t)(int8_t)succ << 8) |
         ((uint32_t)rewarded(counted, d, succ) << 16) | (1u << 24);
}

// Episode statistics of the wave's envs this tick (every lane calls): successes, episode ends,
// env steps, added to wave-uniform running sums.
__device__ __forceinline__ void tally_stats(const bool& live, const int& counted, const int& d, const int& succ,
                                            uint32_t& n_succ, uint32_t& n_end, uint32_t& n_step) {
  const uint64_t bs = __ballot(live && counted && d && succ == 1);
  const uint64_t be = __ballot(live && counted && d);
  const uint64_t bt = __ballot(live && counted);
  n_succ += (uint32_t)__popcll(bs);
  n_end += (uint32_t)__popcll(be);
  n_step += (uint32_t)__popcll(bt);
}
// One lane adds the sums to a stats_part row (no-return atomics: the wave does not wait).
__device__ __forceinline__ void add_stats(const SimView& v, int64_t row, uint32_t n_succ, uint32_t n_end, uint32_t n_step) {
  unsigned long long* r = reinterpret_cast<unsigned long long*>(v.stats_part + 4 * row);
  atomicAdd(r + 0, (unsigned long long)n_succ);
  atomicAdd(r + 1, (unsigned long long)n_end);
  atomicAdd(r + 2, (unsigned long long)n_step);
}

// ---- cells cleared this episode ---------------------------------------------------------------

// f(cell) for every cell of the 256-bit mask m, in ascending order.
template <class F>
__device__ __forceinline__ void for_each_masked_cell(const uint32_t (&m)[8], F f) {
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    uint32_t mm = m[w];
    while (mm) {
      f(w * 32 + __ffs(mm) - 1);
      mm &= mm - 1;
    }
  }
}

// The one-tick kernels: the row is pool[scenario], the mask says which cells are gone.
__device__ __forceinline__ void apply_mask_to_row(const uint32_t (&m)[8], uint8_t* g) {
  for_each_masked_cell(m, [&](int c) __attribute__((always_inline)) { g[c] = 0; });
}

// Sizes (CS, C), like the other scalars of this header, come by reference: read where they are
// used, as when these loops were written out in the kernels, they compile to the same code
// there (by value, rollout_split_kernel's continuous pipeline came out with other registers).

// One LDS row of CS bytes to another as dwords, 12 reads in flight at a time.
__device__ __forceinline__ void copy_row_words(uint32_t* dst, const uint32_t* src, const int& CS) {
  for (int q0 = 0; q0 < (CS >> 2); q0 += 12) {
    uint32_t w[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) w[j] = q0 + j < (CS >> 2) ? src[q0 + j] : 0u;
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (q0 + j < (CS >> 2)) dst[q0 + j] = w[j];
  }
}

// The K-tick kernels keep each env's grid row in LDS for the whole unit and never carry the
// mask: cells are only ever cleared, so the mask is {c : pristine[c] != 0 and grid[c] == 0}
// (cleared_mask below).  The list is what makes an auto-reset cheap: up to 3 cell ids (bits
// 0-23), their count (bits 24-25), bit 31 = more than that were cleared (restore the row).
struct ClearList {
  uint32_t w = 0;
  __device__ __forceinline__ bool overflowed() const { return (w >> 31) != 0; }
  __device__ __forceinline__ uint32_t count() const { return (w >> 24) & 3; }
  __device__ __forceinline__ int cell(int i) const { return (int)((w >> (8 * i)) & 0xffu); }
  // the next push still records its cell (callers that keep a parallel word per listed cell)
  __device__ __forceinline__ bool has_room() const { return !overflowed() && count() < 3; }
  __device__ __forceinline__ void clear() { w = 0; }
  // Once overflowed the list stays overflowed until the episode restarts.
  __device__ __forceinline__ void push(int c) {
    const uint32_t nc = count();
    w = overflowed() ? w
        : nc < 3 ? ((w & 0x00ffffffu) | ((uint32_t)c << (8 * nc)) | ((nc + 1) << 24)) : (1u << 31);
  }
  // Grid row g back to the pristine row: the listed cells (kind(i, c) gives the i-th one's
  // initial kind), or all CS bytes after an overflow.
  template <class K>
  __device__ __forceinline__ void restore(uint8_t* g, const uint32_t* pristine, const int& CS, K kind) const {
    if (overflowed()) {
      copy_row_words(reinterpret_cast<uint32_t*>(g), pristine, CS);
    } else {
      const int nc = (int)count();
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i < nc) {
          const int c = cell(i);
          g[c] = kind(i, c);
        }
    }
  }
  __device__ __forceinline__ void restore(uint8_t* g, const uint32_t* pristine, const int& CS) const {
    const uint8_t* pr = reinterpret_cast<const uint8_t*>(pristine);
    restore(g, pristine, CS, [&](int, int c) __attribute__((always_inline)) { return pr[c]; });
  }
};

// Taking a tile over: the mask's cells leave the freshly loaded row and fill the list.
__device__ __forceinline__ void apply_mask_to_row(const uint32_t (&m)[8], uint8_t* g, ClearList& clr) {
  for_each_masked_cell(m, [&](int c) __attribute__((always_inline)) {
    g[c] = 0;
    clr.push(c);
  });
}

// pool[scenario] (L2-resident) into the env's pristine row and its grid row, 4 x 16 B in flight.
__device__ __forceinline__ void load_pool_row(const uint4* pool_row, uint32_t* pristine, uint32_t* grid, const int& CS) {
  const int nchunk = CS >> 4;
  for (int q0 = 0; q0 < nchunk; q0 += 4) {
    uint4 cq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q0 + j < nchunk) cq[j] = pool_row[q0 + j];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q0 + j < nchunk) {
        const int q = 4 * (q0 + j);
        pristine[q + 0] = grid[q + 0] = cq[j].x;
        pristine[q + 1] = grid[q + 1] = cq[j].y;
        pristine[q + 2] = grid[q + 2] = cq[j].z;
        pristine[q + 3] = grid[q + 3] = cq[j].w;
      }
  }
}

// This episode's mask from the rows: pristine byte nonzero and current byte zero, 4 cells per
// word (SWAR); fully unrolled so every mask word index is static.
__device__ __forceinline__ void cleared_mask(const uint32_t* pristine, const uint32_t* grid, const int& C, uint32_t (&m)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = 0u;
#pragma unroll
  for (int q = 0; q < CRAFT_MAX_CELLS / 4; ++q)
    if (q < (C + 3) >> 2)
      m[q >> 3] |= byte_tops(nonzero_bytes(pristine[q]) & zero_bytes(grid[q])) << (4 * (q & 7));
}

// The env's state, inventory (8 words) and mask (8 words) back to HBM.  sc1: write-through
// stores, the hand-off form of MI355X_MICROARCH.md "Valid forms" ({sc1 stores} -> every
// storing wave's s_waitcnt vmcnt(0) -> one lane's flag), which leaves this XCD's L2 alone.
__device__ __forceinline__ void publish_state(const SimView& v, const int64_t& slot, const uint64_t& st, const uint32_t* ivw,
                                              const uint32_t* m, bool sc1) {
  if (sc1) {
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t inv_r = __builtin_amdgcn_make_buffer_rsrc(v.inv, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t msk_r = __builtin_amdgcn_make_buffer_rsrc(v.mask, 0, 0x7fffffff, 0x00020000);
    const int off = (int)(slot * 32);
    __hip_atomic_store((gu64*)(v.state + slot), (unsigned long long)st, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_raw_buffer_store_b128(u4v{ivw[0], ivw[1], ivw[2], ivw[3]}, inv_r, off, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b128(u4v{ivw[4], ivw[5], ivw[6], ivw[7]}, inv_r, off + 16, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b128(u4v{m[0], m[1], m[2], m[3]}, msk_r, off, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b128(u4v{m[4], m[5], m[6], m[7]}, msk_r, off + 16, 0, 16);
  } else {
    v.state[slot] = st;
    v.inv[2 * slot] = make_uint4(ivw[0], ivw[1], ivw[2], ivw[3]);
    v.inv[2 * slot + 1] = make_uint4(ivw[4], ivw[5], ivw[6], ivw[7]);
    v.mask[2 * slot] = make_uint4(m[0], m[1], m[2], m[3]);
    v.mask[2 * slot + 1] = make_uint4(m[4], m[5], m[6], m[7]);
  }
}

}  // namespace craft
