// craft_checks_rollout_stream.h — what craft_rollout_stream refuses, once for both libraries, in
// the manner of craft_checks.h (whose Facts, refuse and ring_slots_aligned it uses): the check
// reads only, writes `msg` only when it refuses, and the order of its tests is part of the ABI's
// behaviour.
#pragma once
#include "craft_checks.h"

namespace craft_host {

inline int check_rollout_stream(const Facts& f, const craft_rollout_stream_args_t* x, std::string& msg) {
  if (x->flags != CRAFT_STEP_AUTORESET)
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_stream: flags must be CRAFT_STEP_AUTORESET");
  if (x->n_ticks < 0 || x->ring < 1 || x->tick0 < 0)
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_stream: need n_ticks >= 0, ring >= 1, tick0 >= 0");
  if (!ring_slots_aligned(f, x->obs, x->ring))
    return refuse(msg, CRAFT_EINVAL, "craft_rollout_stream: every obs ring slot must be 16-byte aligned");
  if (f.queue_count == 0 || !f.queue_begun)
    return refuse(msg, CRAFT_EINVAL,
                  "craft_rollout_stream: craft_episode_begin has not put the slots on the queue");
  return CRAFT_OK;
}

}  // namespace craft_host
