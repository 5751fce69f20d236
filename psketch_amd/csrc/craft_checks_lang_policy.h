// craft_checks_lang_policy.h — what craft_policy_ask, craft_step_lang_policy and
// craft_step_lang_policy_stream refuse, once for both libraries, in the manner of
// craft_checks_policy.h (whose check_policy_head it uses): a check reads only, writes `msg` only
// when it refuses, and the order of its tests is part of the ABI's behaviour.  The heads' own
// refusals come first (the main head, then the alt head), then actions (the actions are the
// head's), then the alt head against alt_actions and use_alt, then whatever the wrapped entry
// point refuses, with that entry point's message.
#pragma once
#include "craft_checks_lang_stream.h"
#include "craft_checks_policy.h"

namespace craft_host {

// craft_policy_ask: head->mode and head->seed are not read, so only the logits are checked.
inline int check_policy_ask(const craft_policy_head_t* h, float threshold, const uint8_t* ask_out, std::string& msg) {
  if (!h) return refuse(msg, CRAFT_EINVAL, "craft_policy_ask: head is NULL");
  if (!h->logits) return refuse(msg, CRAFT_EINVAL, "craft_policy_ask: head.logits is NULL");
  if (reinterpret_cast<uintptr_t>(h->logits) & 7u)
    return refuse(msg, CRAFT_EINVAL, "craft_policy_ask: head.logits must be 8-byte aligned");
  if (!ask_out) return refuse(msg, CRAFT_EINVAL, "craft_policy_ask: ask_out is NULL");
  if (!(threshold >= 0.0f && threshold <= 1.0f))
    return refuse(msg, CRAFT_EINVAL, "craft_policy_ask: threshold must be in [0, 1]");
  return CRAFT_OK;
}

// The two heads against a craft_lang_step_args_t, for `who`.  With an alt head the wrapped check
// then sees the step without use_alt: the alt head stands where alt_actions would.
inline int check_lang_heads(const craft_lang_step_args_t& p, const craft_policy_head_t* h,
                            const craft_policy_head_t* alt, const char* who, craft_lang_step_args_t& wrapped,
                            std::string& msg) {
  if (const int rc = check_policy_head(h, who, msg)) return rc;
  if (alt) {
    const std::string alt_who = std::string(who) + ": alt_head";
    if (const int rc = check_policy_head(alt, alt_who.c_str(), msg)) return rc;
  }
  auto no = [&](const char* text) {
    msg = std::string(who) + text;
    return CRAFT_EINVAL;
  };
  if (p.actions) return no(": actions must be NULL (the actions are the head's)");
  if (alt && p.alt_actions) return no(": alt_actions must be NULL with an alt_head (the alt actions are its)");
  if (alt && !p.use_alt) return no(": alt_head needs use_alt");
  wrapped = p;
  if (alt) wrapped.use_alt = nullptr;
  return CRAFT_OK;
}

// craft_step_lang_policy: then check_step_lang.
inline int check_step_lang_policy(const Facts& f, const craft_lang_step_args_t* x, const craft_policy_head_t* h,
                                  const craft_policy_head_t* alt, std::string& msg) {
  craft_lang_step_args_t w;
  if (const int rc = check_lang_heads(*x, h, alt, "craft_step_lang_policy", w, msg)) return rc;
  return check_step_lang(f, &w, msg);
}

// craft_step_lang_policy_stream: then check_step_lang_stream.
inline int check_step_lang_policy_stream(const Facts& f, const craft_lang_stream_step_args_t* x,
                                         const craft_policy_head_t* h, const craft_policy_head_t* alt,
                                         std::string& msg) {
  craft_lang_stream_step_args_t w = *x;
  if (const int rc = check_lang_heads(x->step, h, alt, "craft_step_lang_policy_stream", w.step, msg)) return rc;
  return check_step_lang_stream(f, &w, msg);
}

}  // namespace craft_host
