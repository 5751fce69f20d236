// craft_checks_lang_stream.h — what craft_step_lang_stream refuses, once for both libraries, in
// the manner of craft_checks.h (whose Facts, refuse, aligned16 and bfs_queue it uses): the check
// reads only, writes `msg` only when it refuses, and the order of its tests is part of the ABI's
// behaviour.  The HIP library's own refusal (a captured launch while pool rows wait for their
// teacher-table entries) is tick_plan's, as for the other ticks.
#pragma once
#include "craft_checks.h"

namespace craft_host {

inline int check_step_lang_stream(const Facts& f, const craft_lang_stream_step_args_t* x, std::string& msg) {
  if (x->step.flags != 0)
    return refuse(msg, CRAFT_EINVAL, "craft_step_lang_stream: step.flags must be 0 (the queue is the restart)");
  if (x->step.use_alt && !x->step.alt_actions)
    return refuse(msg, CRAFT_EINVAL, "craft_step_lang_stream: use_alt needs alt_actions");
  if (x->step.obs && !aligned16(x->step.obs))
    return refuse(msg, CRAFT_EINVAL, "craft_step_lang_stream: obs must be 16-byte aligned");
  if (f.queue_count == 0 || !f.queue_begun)
    return refuse(msg, CRAFT_EINVAL,
                  "craft_step_lang_stream: craft_episode_begin has not put the slots on the queue");
  return x->step.label_out ? bfs_queue(f, "craft_step_lang_stream", msg) : CRAFT_OK;
}

}  // namespace craft_host
