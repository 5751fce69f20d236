"""What craft_policy_actions, craft_step_policy and craft_step_policy_stream refuse
(psketch_amd/csrc/craft_checks_policy.h), one row per refusal in the manner of
tests/refusal_cases.py, whose handles, Row and check_row these use, and rows in which two
conditions fail at once: the head's refusals come first, then step.actions, then what the wrapped
entry point refuses, with its own text.  tests/test_policy_head_cpu.py runs the table on the CPU
variant, tests/test_gpu_policy_head.py on the HIP library.  Both must refuse every row before any
work, with this status and this text, and leave the handle as it was; check_still_steps then runs
a tick on it."""
import ctypes

import torch

from psketch_amd import _native as N
from tests.refusal_cases import N_ENVS, Row, _bfs

HANDLES = ("base", "queued", "begun", "big")
_E, _n = N.EINVAL, N_ENVS
ENTRIES = ("craft_policy_actions", "craft_step_policy", "craft_step_policy_stream")


def logits(c, misalign=False):
    base = torch.zeros(6 * _n + 4, dtype=torch.float32, device=c.sim.device)
    assert base.data_ptr() % 8 == 0
    c._keep_logits = base
    return base.data_ptr() + (4 if misalign else 0)


def head(c, null_logits=False, mode=N.HEAD_ARGMAX, misalign=False):
    h = N.craft_policy_head_t()
    h.logits = None if null_logits else logits(c, misalign)
    h.mode = mode
    return h


def raw(c, entry, hd="ok", actions=False, flags=None, teach=False, clone_without_ref=False, misaligned_obs=False,
        null_out=False, **head_kw):
    """Straight to the library: `entry` with a valid call but for what the arguments spoil."""
    hp = None if hd is None else ctypes.byref(head(c, **head_kw))
    acts = c.t(_n)
    c._keep = [acts]
    if entry == "craft_policy_actions":
        return c.L.craft_policy_actions(c.h, hp, 0, None if null_out else acts.data_ptr(), c.stream())
    stream = entry == "craft_step_policy_stream"
    args = N.craft_stream_step_args_t() if stream else N.craft_step_args_t()
    st = args.step if stream else args
    st.flags = (N.STEP_AUTORESET if stream else 0) if flags is None else flags
    if actions:
        st.actions = acts.data_ptr()
    if clone_without_ref:
        bc = c.t(_n, dtype=torch.uint8)
        c._keep.append(bc)
        st.behavior_clone = bc.data_ptr()
    if misaligned_obs:
        obs = c.misaligned(_n, c.F)
        c._keep.append(obs)
        st.obs = obs.data_ptr()
    labels = c.t(_n)
    c._keep.append(labels)
    if stream:
        if teach:
            args.label_out = labels.data_ptr()
        return c.L.craft_step_policy_stream(c.h, ctypes.byref(args), hp, c.stream())
    return c.L.craft_step_policy(c.h, ctypes.byref(args), hp, labels.data_ptr() if teach else None, c.stream())


def _head_rows(entry, handle):
    w = entry
    return [
        (f"{w}-null-head", entry, handle, lambda c: raw(c, entry, hd=None), w + ": head is NULL"),
        (f"{w}-null-logits", entry, handle, lambda c: raw(c, entry, null_logits=True), w + ": head.logits is NULL"),
        (f"{w}-mode2", entry, handle, lambda c: raw(c, entry, mode=2),
         w + ": head.mode must be CRAFT_HEAD_ARGMAX (0) or CRAFT_HEAD_SAMPLE (1)"),
        (f"{w}-mode-1", entry, handle, lambda c: raw(c, entry, mode=-1),
         w + ": head.mode must be CRAFT_HEAD_ARGMAX (0) or CRAFT_HEAD_SAMPLE (1)"),
        (f"{w}-misaligned", entry, handle, lambda c: raw(c, entry, misalign=True),
         w + ": head.logits must be 8-byte aligned"),
        # two at once: the earlier test answers
        (f"{w}-order-logits-mode", entry, handle, lambda c: raw(c, entry, null_logits=True, mode=9),
         w + ": head.logits is NULL"),
        (f"{w}-order-mode-align", entry, handle, lambda c: raw(c, entry, mode=9, misalign=True),
         w + ": head.mode must be CRAFT_HEAD_ARGMAX (0) or CRAFT_HEAD_SAMPLE (1)"),
    ]


_P, _S, _Q = ENTRIES
_ACT_S = _S + ": step.actions must be NULL (the actions are the head's)"
_ACT_Q = _Q + ": step.actions must be NULL (the actions are the head's)"
_rows = [
    *_head_rows(_P, "base"), *_head_rows(_S, "base"), *_head_rows(_Q, "begun"),
    (_P + "-null-out", _P, "base", lambda c: raw(c, _P, null_out=True), _P + ": actions_out is NULL"),
    (_S + "-actions", _S, "base", lambda c: raw(c, _S, actions=True), _ACT_S),
    (_S + "-actions-teach", _S, "base", lambda c: raw(c, _S, actions=True, teach=True), _ACT_S),
    (_Q + "-actions", _Q, "begun", lambda c: raw(c, _Q, actions=True), _ACT_Q),
    # through the binding: logits and actions together
    (_S + "-binding-actions", _S, "base",
     lambda c: c.sim.step(c.t(_n), logits=c.t(_n, 6, dtype=torch.float32)), _ACT_S),
    (_Q + "-binding-actions", _Q, "begun",
     lambda c: c.sim.step_stream(c.t(_n), logits=c.t(_n, 6, dtype=torch.float32)), _ACT_Q),
    (_S + "-binding-mode", _S, "base", lambda c: c.sim.step(logits=c.t(_n, 6, dtype=torch.float32), head=5),
     _S + ": head.mode must be CRAFT_HEAD_ARGMAX (0) or CRAFT_HEAD_SAMPLE (1)"),
    # what the wrapped entry points refuse, with their texts
    (_S + "-obs", _S, "base", lambda c: raw(c, _S, misaligned_obs=True), "craft_step: obs must be 16-byte aligned"),
    (_S + "-clone", _S, "base", lambda c: raw(c, _S, clone_without_ref=True),
     "craft_step_ex: behavior_clone needs ref_actions"),
    (_S + "-teach-bfs", _S, "big", lambda c: raw(c, _S, teach=True), _bfs("craft_step_teach")),
    (_Q + "-flags", _Q, "begun", lambda c: raw(c, _Q, flags=0),
     "craft_step_stream: step.flags must be CRAFT_STEP_AUTORESET"),
    (_Q + "-no-queue", _Q, "base", lambda c: raw(c, _Q),
     "craft_step_stream: craft_episode_begin has not put the slots on the queue"),
    (_Q + "-not-begun", _Q, "queued", lambda c: raw(c, _Q),
     "craft_step_stream: craft_episode_begin has not put the slots on the queue"),
    (_Q + "-teach-bfs", _Q, "big", lambda c: raw(c, _Q, teach=True), _bfs("craft_step_stream")),
    (_Q + "-obs", _Q, "begun", lambda c: raw(c, _Q, misaligned_obs=True), "craft_step: obs must be 16-byte aligned"),
    # order: the head, then step.actions, then the wrapped entry point
    (_S + "-order-head-actions", _S, "base", lambda c: raw(c, _S, mode=3, actions=True),
     _S + ": head.mode must be CRAFT_HEAD_ARGMAX (0) or CRAFT_HEAD_SAMPLE (1)"),
    (_S + "-order-actions-obs", _S, "base", lambda c: raw(c, _S, actions=True, misaligned_obs=True), _ACT_S),
    (_Q + "-order-actions-flags", _Q, "begun", lambda c: raw(c, _Q, actions=True, flags=0), _ACT_Q),
]
ROWS = [Row("policy_head-" + i, e, h, call, _E, msg) for i, e, h, call, msg in _rows]


def check_still_steps(c):
    """After the refusals: each of the three entry points accepts a valid call on the handle (the
    stream tick where its queue was begun), and nothing latches."""
    sim = c.sim
    L = torch.full((_n, 6), float("-inf"), dtype=torch.float32, device=sim.device)
    L[:, 2] = 1.0                                         # every other action masked: both modes give 2
    acts = sim.policy_actions(L, "argmax")
    assert (acts.cpu() == 2).all()
    rec = c.t(_n)
    if c.name == "begun":
        sim.step_stream(logits=L, head="sample", head_seed=1, tick=0, action_record=rec)
    elif c.name != "big":
        sim.step(logits=L, head="argmax", tick=0, action_record=rec,
                 labels=c.t(_n) if c.name == "base" else None)
    sim.check()
    if c.name != "big":
        assert ((rec.cpu() == 2) | (rec.cpu() == -1)).all()
