"""What craft_episode_summary refuses (psketch_amd/csrc/craft_checks_episode_summary.h), one row per
refusal in the manner of tests/rollout_stream_refusal_cases.py, whose handles, Row and check_row
these use, and rows in which two conditions fail at once: the order of the tests is part of the
behaviour.  tests/test_episode_summary_cpu.py runs the table on the CPU variant,
tests/test_gpu_episode_summary.py on the HIP library.  Both must refuse every row before any work,
with this status and this text, and leave the handle as it was."""
import ctypes

import torch

from psketch_amd import _native as N
from tests.refusal_cases import N_ENVS, QUEUE, Row, _bfs

HANDLES = ("base", "queued", "begun", "big")
_E, _n = N.EINVAL, N_ENVS
_W = "craft_episode_summary"
REQUIRED = ("episode_end", "end_pose", "success", "length_out", "success_out", "end_pose_out", "flags_out")


def raw(c, ticks=2, count=QUEUE, null=(), actions=False, record=False, run=False, now=False, distance=False):
    """Straight to the library with tiny tensors: the required pointers set but for those named
    in `null`, the optional ones only where asked."""
    T = c.sim.config.max_timesteps
    rows = max(ticks, 1)
    bufs = {"episode_end": c.t(rows, _n, fill=-1), "end_pose": c.t(rows, _n, fill=-1),
            "success": c.t(rows, _n, dtype=torch.int8, fill=-1), "length_out": c.t(QUEUE),
            "success_out": c.t(QUEUE, dtype=torch.int8), "end_pose_out": c.t(QUEUE), "flags_out": c.t(2)}
    if record:
        bufs["action_record"] = c.t(rows, _n, fill=-1)
    if actions:
        bufs["actions_out"] = c.t(QUEUE, T)
    if run:
        bufs["run"] = c.t(_n)
    if now:
        bufs["episode_now"] = c.t(_n)
    if distance:
        bufs["distance_out"] = c.t(QUEUE)
    c._keep = bufs
    args = N.craft_episode_summary_args_t()
    for k, v in bufs.items():
        if k not in null:
            setattr(args, k, v.data_ptr())
    args.ticks, args.count = ticks, count
    return c.L.craft_episode_summary(c.h, ctypes.byref(args), c.stream())


_NULL = _W + ": args is NULL"
_REQ = (_W + ": episode_end, end_pose, success, length_out, success_out, end_pose_out and flags_out are "
        "required")
_TICKS = _W + ": ticks must be >= 0"
_QUEUE = _W + ": no episode queue installed (craft_episode_queue)"
_COUNT = _W + ": count must be 1 .. the queue's length"
_ACTIONS = _W + ": actions_out needs action_record"
_NOW = _W + ": run with action_record needs episode_now"
_rows = [
    ("null-args", "begun", lambda c: c.L.craft_episode_summary(c.h, None, c.stream()), _NULL),
    *[("null-" + f, "begun", lambda c, f=f: raw(c, null=(f,)), _REQ) for f in REQUIRED],
    ("ticks", "begun", lambda c: raw(c, ticks=-1), _TICKS),
    ("no-queue", "base", lambda c: raw(c), _QUEUE),
    ("count0", "queued", lambda c: raw(c, count=0), _COUNT),
    ("count-neg", "begun", lambda c: raw(c, count=-3), _COUNT),
    ("count-past", "begun", lambda c: raw(c, count=QUEUE + 1), _COUNT),
    ("actions", "begun", lambda c: raw(c, actions=True), _ACTIONS),
    ("run-now", "begun", lambda c: raw(c, record=True, run=True), _NOW),
    ("bfs", "big", lambda c: raw(c, distance=True), _bfs(_W)),
    # through the binding: it allocates actions only with a record, so the missing episode_now
    ("binding-run-now", "begun",
     lambda c: c.sim.episode_summary(c.t(2, _n, fill=-1), c.t(2, _n, fill=-1), c.t(2, _n, dtype=torch.int8, fill=-1),
                                     action_record=c.t(2, _n, fill=-1), run=c.t(_n)), _NOW),
    ("binding-bfs", "big",
     lambda c: c.sim.episode_summary(c.t(2, _n, fill=-1), c.t(2, _n, fill=-1), c.t(2, _n, dtype=torch.int8, fill=-1)),
     _bfs(_W)),
    # two at once: the earlier test of the list answers
    ("order-required-ticks", "begun", lambda c: raw(c, ticks=-1, null=("success",)), _REQ),
    ("order-ticks-queue", "base", lambda c: raw(c, ticks=-1), _TICKS),
    ("order-queue-count", "base", lambda c: raw(c, count=0), _QUEUE),
    ("order-count-actions", "begun", lambda c: raw(c, count=0, actions=True), _COUNT),
    ("order-actions-now", "begun", lambda c: raw(c, actions=True, run=True), _ACTIONS),
    ("order-now-bfs", "big", lambda c: raw(c, record=True, run=True, distance=True), _NOW),
]
ROWS = [Row("episode_summary-" + i, _W, h, call, _E, msg) for i, h, call, msg in _rows]


def check_accepts(c):
    """What the rows' neighbours accept: a queue that was installed but never begun, no ticks,
    and every optional output left out."""
    assert raw(c, ticks=0) == N.OK
    assert raw(c, ticks=2) == N.OK
    assert raw(c, ticks=2, record=True, actions=True, run=True, now=True, count=1) == N.OK
    c.sim.check()
