// craft_checks_episode_summary.h — what craft_episode_summary refuses, once for both libraries,
// in the manner of craft_checks_rollout_stream.h (craft_checks.h's Facts, refuse and bfs_queue):
// the check reads only, writes `msg` only when it refuses, and the order of its tests is part of
// the ABI's behaviour.  A NULL args is refused here too, so that it has a text like the rest.
#pragma once
#include "craft_checks.h"

namespace craft_host {

inline int check_episode_summary(const Facts& f, const craft_episode_summary_args_t* x, std::string& msg) {
  if (!x) return refuse(msg, CRAFT_EINVAL, "craft_episode_summary: args is NULL");
  if (!x->episode_end || !x->end_pose || !x->success || !x->length_out || !x->success_out || !x->end_pose_out ||
      !x->flags_out)
    return refuse(msg, CRAFT_EINVAL,
                  "craft_episode_summary: episode_end, end_pose, success, length_out, success_out, end_pose_out "
                  "and flags_out are required");
  if (x->ticks < 0) return refuse(msg, CRAFT_EINVAL, "craft_episode_summary: ticks must be >= 0");
  if (f.queue_count == 0)
    return refuse(msg, CRAFT_EINVAL, "craft_episode_summary: no episode queue installed (craft_episode_queue)");
  if (x->count < 1 || x->count > f.queue_count)
    return refuse(msg, CRAFT_EINVAL, "craft_episode_summary: count must be 1 .. the queue's length");
  if (x->actions_out && !x->action_record)
    return refuse(msg, CRAFT_EINVAL, "craft_episode_summary: actions_out needs action_record");
  if (x->run && x->action_record && !x->episode_now)
    return refuse(msg, CRAFT_EINVAL, "craft_episode_summary: run with action_record needs episode_now");
  if (x->distance_out)
    if (const int rc = bfs_queue(f, "craft_episode_summary", msg)) return rc;
  return CRAFT_OK;
}

}  // namespace craft_host
