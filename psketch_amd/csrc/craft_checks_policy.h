// craft_checks_policy.h — what craft_policy_actions, craft_step_policy and craft_step_policy_stream
// refuse, once for both libraries, in the manner of craft_checks.h (whose Facts and refuse it uses):
// a check reads only, writes `msg` only when it refuses, and the order of its tests is part of
// the ABI's behaviour.  The head's own refusals come first, then step.actions (the actions are the
// head's), then whatever the wrapped entry point refuses, with that entry point's message.
#pragma once
#include "craft_checks.h"

namespace craft_host {

// The craft_policy_head_t of `who` (an entry point's name).
inline int check_policy_head(const craft_policy_head_t* h, const char* who, std::string& msg) {
  auto no = [&](const char* text) {
    msg = std::string(who) + text;
    return CRAFT_EINVAL;
  };
  if (!h) return no(": head is NULL");
  if (!h->logits) return no(": head.logits is NULL");
  if (h->mode != CRAFT_HEAD_ARGMAX && h->mode != CRAFT_HEAD_SAMPLE)
    return no(": head.mode must be CRAFT_HEAD_ARGMAX (0) or CRAFT_HEAD_SAMPLE (1)");
  if (reinterpret_cast<uintptr_t>(h->logits) & 7u) return no(": head.logits must be 8-byte aligned");
  return CRAFT_OK;
}

inline int check_policy_actions(const craft_policy_head_t* h, const int32_t* actions_out, std::string& msg) {
  if (const int rc = check_policy_head(h, "craft_policy_actions", msg)) return rc;
  if (!actions_out) return refuse(msg, CRAFT_EINVAL, "craft_policy_actions: actions_out is NULL");
  return CRAFT_OK;
}

// craft_step_policy: then check_step (label_out NULL) or check_step_teach.
inline int check_step_policy(const Facts& f, const craft_step_args_t* x, const craft_policy_head_t* h,
                             const int32_t* label_out, std::string& msg) {
  if (const int rc = check_policy_head(h, "craft_step_policy", msg)) return rc;
  if (x->actions)
    return refuse(msg, CRAFT_EINVAL, "craft_step_policy: step.actions must be NULL (the actions are the head's)");
  return label_out ? check_step_teach(f, x, msg) : check_step(x, msg);
}

// craft_step_policy_stream: then check_step_stream.
inline int check_step_policy_stream(const Facts& f, const craft_stream_step_args_t* x, const craft_policy_head_t* h,
                                    std::string& msg) {
  if (const int rc = check_policy_head(h, "craft_step_policy_stream", msg)) return rc;
  if (x->step.actions)
    return refuse(msg, CRAFT_EINVAL,
                  "craft_step_policy_stream: step.actions must be NULL (the actions are the head's)");
  return check_step_stream(f, x, msg);
}

}  // namespace craft_host
