// craft_checks_rollout_replay.h — what craft_episode_actions and craft_rollout_replay refuse, once
// for both libraries, in the manner of craft_checks_rollout_stream.h: a check reads only, writes
// `msg` only when it refuses, and the order of its tests is part of the ABI's behaviour.  (Whether
// a tape row is valid is each library's own test, like a queue entry's; only its message is
// shared, tape_row_invalid.)
#pragma once
#include "craft_checks_rollout_stream.h"

namespace craft_host {

inline int check_episode_actions(const Facts& f, const int32_t* actions, int64_t count, std::string& msg) {
  if (f.queue_count == 0)
    return refuse(msg, CRAFT_EINVAL, "craft_episode_actions: no episode queue installed (craft_episode_queue)");
  if (!actions && count == 0) return CRAFT_OK;           // drops the tape
  if (!actions || count != f.queue_count) {
    msg = "craft_episode_actions: need one row per queue entry (" + std::to_string(f.queue_count) +
          "), or NULL and 0 to drop the tape";
    return CRAFT_EINVAL;
  }
  return CRAFT_OK;
}

// craft_episode_actions' refusal of a tape whose lowest invalid row is `index`.
inline int tape_row_invalid(uint64_t index, std::string& msg) {
  msg = "craft_episode_actions: entry " + std::to_string(index) +
        " is invalid (1..max_timesteps actions in 0..5 then -1, ending in its only STOP or max_timesteps long)";
  return CRAFT_EINVAL;
}

// have_tape: a tape is installed for the current queue.
inline int check_rollout_replay(const Facts& f, const craft_rollout_replay_args_t* x, bool have_tape,
                                std::string& msg) {
  if (const int rc = check_rollout_stream(f, &x->roll, msg)) {
    // craft_rollout_stream's refusals, in its order, under this entry point's name
    const std::string from = "craft_rollout_stream";
    if (msg.compare(0, from.size(), from) == 0) msg.replace(0, from.size(), "craft_rollout_replay");
    return rc;
  }
  if (x->roll.actions)
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_replay: roll.actions must be NULL (the actions are the tape's)");
  if (!have_tape)
    return refuse(msg, CRAFT_EINVAL,
                  "craft_rollout_replay: no actions installed for the current queue (craft_episode_actions)");
  return CRAFT_OK;
}

}  // namespace craft_host
