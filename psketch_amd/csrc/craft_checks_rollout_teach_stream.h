// craft_checks_rollout_teach_stream.h — what craft_rollout_teach_stream refuses, once for both
// libraries, in the manner of craft_checks_rollout_stream.h: the check reads only, writes `msg`
// only when it refuses, and the order of its tests is part of the ABI's behaviour.
#pragma once
#include "craft_checks.h"

namespace craft_host {

inline int check_rollout_teach_stream(const Facts& f, const craft_rollout_teach_stream_args_t* x, std::string& msg) {
  const craft_rollout_teach_args_t& t = x->teach;
  if (t.flags != CRAFT_STEP_AUTORESET)
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_teach_stream: teach.flags must be CRAFT_STEP_AUTORESET");
  if (t.n_ticks < 0 || t.ring < 1 || t.tick0 < 0)
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_teach_stream: need n_ticks >= 0, ring >= 1, tick0 >= 0");
  if (const int rc = bfs_queue(f, "craft_rollout_teach_stream", msg)) return rc;
  if ((t.label_actions != 0 || t.behavior_clone != nullptr) && !t.label_in)
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_teach_stream: label_actions / behavior_clone need label_in");
  if (!ring_slots_aligned(f, t.obs, t.ring))
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_teach_stream: every obs ring slot must be 16-byte aligned");
  if (f.queue_count == 0 || !f.queue_begun)
    return refuse(msg, CRAFT_EINVAL,
                  "craft_rollout_teach_stream: craft_episode_begin has not put the slots on the queue");
  return CRAFT_OK;
}

}  // namespace craft_host
