// craft_launch.h — the launchers craft_sim.hip calls, declared once.  Every translation unit that
// defines one includes this header, so caller and definition read the same prototype.
#pragma once
#include "craft_device.h"

namespace craft {

// craft_tile.hip
hipError_t launch_tile(int mode, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                       hipStream_t st);
// craft_tick_teach.hip (head: the policy head's instantiations, a.logits set)
hipError_t launch_tick_teach(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                             hipStream_t st, bool head = false);
hipError_t launch_tick2(int tl, int nw, const SimView& v, const TileArgs& a, size_t lds, hipStream_t st,
                        bool head = false);
size_t tick2_lds_bytes(int tl, int nw, int GS, int F);
// craft_tick_lang.hip, craft_tick_stream.hip: tl = 0 launches the bare tick
hipError_t launch_tick_lang(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                            hipStream_t st, bool head = false);
hipError_t launch_tick_stream(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                              hipStream_t st, bool head = false);
// craft_tick_policy.hip, craft_tick_policy_stream.hip: where the three launchers above (and launch_tile's
// MODE_TICK_HEAD) find the tile kernel's policy-head instantiations (tl = 0: the bare tick), and
// craft_policy_actions' kernel
hipError_t launch_tick_head(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                            hipStream_t st);
hipError_t launch_tick_stream_head(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a,
                                   size_t lds, hipStream_t st);
hipError_t launch_policy_actions(const float* logits, int32_t mode, uint64_t seed, int64_t gid0, int64_t tick,
                                 int64_t n, int32_t* actions_out, hipStream_t st);
hipError_t launch_policy_ask(const float* logits, float threshold, int64_t n, uint8_t* ask_out, hipStream_t st);
// craft_tick_lang_policy.hip, craft_tick_lang_policy_stream.hip: the language ticks' head instantiations
// (MODE_LANG_HEAD, MODE_LANG_STREAM_HEAD), found by launch_tick_lang / launch_tick_lang_stream with head set
hipError_t launch_tick_lang_head(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                                 hipStream_t st);
hipError_t launch_tick_lang_stream_head(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a,
                                        size_t lds, hipStream_t st);
// craft_tick_lang_stream.hip
hipError_t launch_tick_lang_stream(int tl, int nw, int win, int tile, const SimView& v, const TileArgs& a, size_t lds,
                                   hipStream_t st, bool head = false);
hipError_t launch_queue_pack(const SimView& v, const int32_t* specs, int64_t count, uint2* out,
                             unsigned long long* first_bad, hipStream_t st);
hipError_t launch_queue_begin(const uint2* entries, int64_t count, int64_t first_gid, int wrap, int64_t n,
                              int32_t* cursor, int32_t* r, hipStream_t st);
// craft_rollout_w3.hip, craft_rollout_teach.hip
hipError_t launch_rollout(int win, int tile, int threads, const SimView& v, const RolloutArgs& a, size_t lds,
                          hipStream_t st);
// craft_rollout_stream.hip: 512 threads on rollout_stream_tile's 32- or 16-env tiles
int rollout_stream_tile(int tile_knob, const SimView& v);
hipError_t launch_rollout_stream(int win, int tile, const SimView& v, const RolloutArgs& a, hipStream_t st);
// craft_rollout_replay.hip: the tape's check-and-pack kernel (rows of T int32 -> `stride` bytes),
// and craft_rollout_stream's shapes with the tape as the action source
hipError_t launch_tape_pack(const int32_t* actions, int64_t count, int T, int stride, uint8_t* out,
                            unsigned long long* first_bad, hipStream_t st);
hipError_t launch_rollout_replay(int win, int tile, const SimView& v, const RolloutArgs& a, hipStream_t st);
hipError_t launch_rollout_teach(int win, int nw, const SimView& v, const RolloutArgs& a, hipStream_t st);
// craft_rollout_teach_stream.hip: the same shape on the episode queue
hipError_t launch_rollout_teach_stream(int win, int nw, const SimView& v, const RolloutArgs& a, hipStream_t st);
// craft_teacher.hip
hipError_t launch_teacher(int nw, int lanes, const SimView& v, const int32_t* slots, const int32_t* tasks,
                          int64_t n, int32_t* act_out, int32_t* len_out, hipStream_t st);
hipError_t launch_distances(int nw, const SimView& v, const int32_t* tasks, const int8_t* success,
                            const int32_t* seqs, int32_t ticks, int64_t n, int32_t* dist_out,
                            uint8_t* is_get_out, int32_t* n_actions_out, int32_t* flags, hipStream_t st);
hipError_t launch_teach_table(int nw, const SimView& v, int32_t first, int32_t count, const int32_t* kinds,
                              hipStream_t st);
// craft_episode_summary.hip: the scan over the slots' record columns, then (a.dist_out set) the
// BFS of the entries the scan left pending
hipError_t launch_episode_summary(int nw, const SimView& v, const SummaryArgs& a, hipStream_t st);
// craft_scenarios.hip
hipError_t launch_scenarios(const SimView& v, const ScenarioArgs& a, hipStream_t st);

}  // namespace craft
