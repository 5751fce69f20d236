"""What craft_policy_ask, craft_step_lang_policy and craft_step_lang_policy_stream refuse
(psketch_amd/csrc/craft_checks_lang_policy.h), one row per refusal in the manner of
tests/refusal_cases.py, whose handles, Row and check_row these use: the main head's refusals, then
the alt head's, then actions, then the alt head against alt_actions and use_alt, then what the
wrapped entry point refuses, with its own text.  tests/test_lang_policy_head_cpu.py runs the table
on the CPU variant, tests/test_gpu_lang_policy_head.py on the HIP library.  Both must refuse every
row before any work, with this status and this text, and leave the handle as it was;
check_still_steps then runs a tick on it."""
import ctypes

import torch

from psketch_amd import _native as N
from tests.policy_head_refusal_cases import head
from tests.refusal_cases import N_ENVS, Row, _bfs

HANDLES = ("base", "queued", "begun", "big")
_E, _n = N.EINVAL, N_ENVS
ENTRIES = ("craft_policy_ask", "craft_step_lang_policy", "craft_step_lang_policy_stream")
_A, _S, _Q = ENTRIES
_MODE = ": head.mode must be CRAFT_HEAD_ARGMAX (0) or CRAFT_HEAD_SAMPLE (1)"


def ask_raw(c, hd="ok", threshold=0.5, null_out=False, **head_kw):
    hp = None if hd is None else ctypes.byref(head(c, **head_kw))
    out = c.t(_n, dtype=torch.uint8)
    c._keep = [out]
    return c.L.craft_policy_ask(c.h, hp, ctypes.c_float(threshold), None if null_out else out.data_ptr(), c.stream())


def raw(c, entry, hd="ok", alt=None, actions=False, alt_actions=False, use_alt=False, flags=0, teach=False,
        misaligned_obs=False, **head_kw):
    """Straight to the library: `entry` with a valid call but for what the arguments spoil.  alt: None
    (no alt head) or the keywords of its head()."""
    hp = None if hd is None else ctypes.byref(head(c, **head_kw))
    keep = [c._keep_logits] if hd is not None and not head_kw.get("null_logits") else []
    ap = None
    if alt is not None:
        ap = ctypes.byref(head(c, **alt))
        keep.append(getattr(c, "_keep_logits", None))
    stream = entry == _Q
    args = N.craft_lang_stream_step_args_t() if stream else N.craft_lang_step_args_t()
    st = args.step if stream else args
    st.flags = flags
    for on_, field, dtype in ((actions, "actions", torch.int32), (alt_actions, "alt_actions", torch.int32),
                              (use_alt, "use_alt", torch.uint8)):
        if on_:
            t = c.t(_n, dtype=dtype)
            keep.append(t)
            setattr(st, field, t.data_ptr())
    if misaligned_obs:
        obs = c.misaligned(_n, c.F)
        keep.append(obs)
        st.obs = obs.data_ptr()
    if teach:
        labels = c.t(_n)
        keep.append(labels)
        st.label_out = labels.data_ptr()
    c._keep = keep
    return getattr(c.L, entry)(c.h, ctypes.byref(args), hp, ap, c.stream())


def _head_rows(entry, handle):
    w = entry
    rows = [
        (f"{w}-null-head", lambda c: raw(c, entry, hd=None), w + ": head is NULL"),
        (f"{w}-null-logits", lambda c: raw(c, entry, null_logits=True), w + ": head.logits is NULL"),
        (f"{w}-mode2", lambda c: raw(c, entry, mode=2), w + _MODE),
        (f"{w}-misaligned", lambda c: raw(c, entry, misalign=True), w + ": head.logits must be 8-byte aligned"),
        (f"{w}-alt-null-logits", lambda c: raw(c, entry, alt=dict(null_logits=True), use_alt=True),
         w + ": alt_head: head.logits is NULL"),
        (f"{w}-alt-mode-1", lambda c: raw(c, entry, alt=dict(mode=-1), use_alt=True), w + ": alt_head" + _MODE),
        (f"{w}-alt-misaligned", lambda c: raw(c, entry, alt=dict(misalign=True), use_alt=True),
         w + ": alt_head: head.logits must be 8-byte aligned"),
        (f"{w}-actions", lambda c: raw(c, entry, actions=True), w + ": actions must be NULL (the actions are the head's)"),
        (f"{w}-alt-head-and-alt-actions", lambda c: raw(c, entry, alt={}, alt_actions=True, use_alt=True),
         w + ": alt_actions must be NULL with an alt_head (the alt actions are its)"),
        (f"{w}-alt-head-without-use-alt", lambda c: raw(c, entry, alt={}), w + ": alt_head needs use_alt"),
        # order: the main head, the alt head, actions, the alt head's arguments, the wrapped entry point
        (f"{w}-order-head-alt", lambda c: raw(c, entry, mode=3, alt=dict(mode=3)), w + _MODE),
        (f"{w}-order-alt-actions", lambda c: raw(c, entry, alt=dict(mode=3), actions=True), w + ": alt_head" + _MODE),
        (f"{w}-order-actions-alt-actions", lambda c: raw(c, entry, actions=True, alt={}, alt_actions=True),
         w + ": actions must be NULL (the actions are the head's)"),
        (f"{w}-order-use-alt-flags", lambda c: raw(c, entry, alt={}, flags=1), w + ": alt_head needs use_alt"),
    ]
    return [(i, entry, handle, call, msg) for i, call, msg in rows]


_rows = [
    (_A + "-null-head", _A, "base", lambda c: ask_raw(c, hd=None), _A + ": head is NULL"),
    (_A + "-null-logits", _A, "base", lambda c: ask_raw(c, null_logits=True), _A + ": head.logits is NULL"),
    (_A + "-misaligned", _A, "base", lambda c: ask_raw(c, misalign=True), _A + ": head.logits must be 8-byte aligned"),
    (_A + "-null-out", _A, "base", lambda c: ask_raw(c, null_out=True), _A + ": ask_out is NULL"),
    (_A + "-threshold-nan", _A, "base", lambda c: ask_raw(c, threshold=float("nan")), _A + ": threshold must be in [0, 1]"),
    (_A + "-threshold-negative", _A, "base", lambda c: ask_raw(c, threshold=-0.25), _A + ": threshold must be in [0, 1]"),
    (_A + "-threshold-above-1", _A, "base", lambda c: ask_raw(c, threshold=1.5), _A + ": threshold must be in [0, 1]"),
    (_A + "-order-out-threshold", _A, "base", lambda c: ask_raw(c, null_out=True, threshold=2.0), _A + ": ask_out is NULL"),
    (_A + "-binding-threshold", _A, "base", lambda c: c.sim.policy_ask(c.t(_n, 6, dtype=torch.float32), 7.0),
     _A + ": threshold must be in [0, 1]"),
    *_head_rows(_S, "base"), *_head_rows(_Q, "begun"),
    # through the binding
    (_S + "-binding-actions", _S, "base", lambda c: c.sim.step_lang(c.t(_n), logits=c.t(_n, 6, dtype=torch.float32)),
     _S + ": actions must be NULL (the actions are the head's)"),
    (_Q + "-binding-alt", _Q, "begun",
     lambda c: c.sim.step_lang_stream(logits=c.t(_n, 6, dtype=torch.float32), alt_logits=c.t(_n, 6, dtype=torch.float32)),
     _Q + ": alt_head needs use_alt"),
    # what the wrapped entry points refuse, with their texts
    (_S + "-flags", _S, "base", lambda c: raw(c, _S, flags=1), "craft_step_lang: flags must be 0 (no auto-reset in this protocol)"),
    (_S + "-use-alt-alone", _S, "base", lambda c: raw(c, _S, use_alt=True), "craft_step_lang: use_alt needs alt_actions"),
    (_S + "-obs", _S, "base", lambda c: raw(c, _S, misaligned_obs=True), "craft_step_lang: obs must be 16-byte aligned"),
    (_S + "-alt-head-obs", _S, "base", lambda c: raw(c, _S, alt={}, use_alt=True, misaligned_obs=True),
     "craft_step_lang: obs must be 16-byte aligned"),
    (_S + "-teach-bfs", _S, "big", lambda c: raw(c, _S, teach=True), _bfs("craft_step_lang")),
    (_Q + "-flags", _Q, "begun", lambda c: raw(c, _Q, flags=1),
     "craft_step_lang_stream: step.flags must be 0 (the queue is the restart)"),
    (_Q + "-use-alt-alone", _Q, "begun", lambda c: raw(c, _Q, use_alt=True), "craft_step_lang_stream: use_alt needs alt_actions"),
    (_Q + "-obs", _Q, "begun", lambda c: raw(c, _Q, misaligned_obs=True), "craft_step_lang_stream: obs must be 16-byte aligned"),
    (_Q + "-no-queue", _Q, "base", lambda c: raw(c, _Q),
     "craft_step_lang_stream: craft_episode_begin has not put the slots on the queue"),
    (_Q + "-not-begun", _Q, "queued", lambda c: raw(c, _Q, alt={}, use_alt=True),
     "craft_step_lang_stream: craft_episode_begin has not put the slots on the queue"),
    (_Q + "-teach-bfs", _Q, "big", lambda c: raw(c, _Q, teach=True), _bfs("craft_step_lang_stream")),
]
ROWS = [Row("lang_policy_head-" + i, e, h, call, _E, msg) for i, e, h, call, msg in _rows]
assert len({r.id for r in ROWS}) == len(ROWS)


def check_still_steps(c):
    """After the refusals: each of the three entry points accepts a valid call on the handle (the
    stream tick where its queue was begun), and nothing latches."""
    sim = c.sim
    L = torch.full((_n, 6), float("-inf"), dtype=torch.float32, device=sim.device)
    L[:, 2] = 1.0                                         # every other action masked: both modes give 2
    A = torch.full((_n, 6), float("-inf"), dtype=torch.float32, device=sim.device)
    A[:, 3] = 1.0
    assert (sim.policy_ask(L, 0.0).cpu() == 0).all()
    assert (sim.policy_ask(torch.zeros_like(L), 0.5).cpu() == 1).all()
    use = (torch.arange(_n, device=sim.device) % 2).to(torch.uint8)
    rec = c.t(_n)
    kw = dict(logits=L, head="sample", head_seed=1, alt_logits=A, alt_head="argmax", use_alt=use, tick=0,
              action_record=rec)
    if c.name == "begun":
        sim.step_lang_stream(**kw)
    elif c.name != "big":
        sim.step_lang(labels=c.t(_n) if c.name == "base" else None, **kw)
    sim.check()
    if c.name != "big":
        r, u = rec.cpu(), use.cpu()
        assert ((r == torch.where(u == 1, 3, 2)) | (r == -1)).all()
