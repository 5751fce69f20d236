"""What craft_rollout_teach_stream refuses (psketch_amd/csrc/craft_checks_rollout_teach_stream.h),
one row per refusal in the manner of tests/rollout_stream_refusal_cases.py, and rows in which two
conditions fail at once: the order of the tests is part of the behaviour.
tests/test_rollout_teach_stream_cpu.py runs the table on the CPU variant,
tests/test_gpu_rollout_teach_stream.py on the HIP library.  Both must refuse every row before any
work, with this status and this text, and leave the handle as it was."""
import ctypes

import torch

from psketch_amd import _native as N
from tests.refusal_cases import N_ENVS, Row, _bfs, make_tables, WORLDS

HANDLES = ("base", "queued", "begun", "big")
_E, _n = N.EINVAL, N_ENVS
_W = "craft_rollout_teach_stream"


def raw(c, flags=N.STEP_AUTORESET, n_ticks=1, ring=1, tick0=0, label_actions=0, obs=None):
    """Straight to the library: the binding always passes CRAFT_STEP_AUTORESET and a ring >= 1."""
    args = N.craft_rollout_teach_stream_args_t()
    t = args.teach
    t.flags, t.n_ticks, t.ring, t.tick0, t.label_actions = flags, n_ticks, ring, tick0, label_actions
    if obs is not None:
        c._keep = obs
        t.obs = obs.data_ptr()
    return c.L.craft_rollout_teach_stream(c.h, ctypes.byref(args), c.stream())


_FLAGS = _W + ": teach.flags must be CRAFT_STEP_AUTORESET"
_NEED = _W + ": need n_ticks >= 0, ring >= 1, tick0 >= 0"
_LABEL = _W + ": label_actions / behavior_clone need label_in"
_OBS = _W + ": every obs ring slot must be 16-byte aligned"
_BEGIN = _W + ": craft_episode_begin has not put the slots on the queue"
_rows = [
    ("flags0", "begun", lambda c: raw(c, flags=0), _FLAGS),
    ("flags3", "begun", lambda c: raw(c, flags=3), _FLAGS),
    ("ticks", "begun", lambda c: raw(c, n_ticks=-1), _NEED),
    ("ring", "begun", lambda c: raw(c, ring=0), _NEED),
    ("tick0", "begun", lambda c: c.sim.rollout_teach_stream(1, tick0=-1), _NEED),
    ("bfs", "big", lambda c: c.sim.rollout_teach_stream(1, labels=c.t(1, _n)), _bfs(_W)),
    ("label-actions", "begun", lambda c: c.sim.rollout_teach_stream(1, label_actions=True), _LABEL),
    ("behavior-clone", "begun",
     lambda c: c.sim.rollout_teach_stream(1, behavior_clone=c.t(_n, dtype=torch.uint8)), _LABEL),
    ("obs", "begun", lambda c: c.sim.rollout_teach_stream(1, obs=c.misaligned(1, _n, c.F)), _OBS),
    ("none", "base", lambda c: c.sim.rollout_teach_stream(1), _BEGIN),
    ("queued", "queued", lambda c: c.sim.rollout_teach_stream(1), _BEGIN),
    # two at once: the earlier test of the list answers
    ("order-flags-ticks", "begun", lambda c: raw(c, flags=0, n_ticks=-1), _FLAGS),
    ("order-ticks-bfs", "big", lambda c: raw(c, n_ticks=-1), _NEED),
    ("order-bfs-label", "big", lambda c: raw(c, label_actions=1), _bfs(_W)),
    ("order-label-obs", "begun", lambda c: raw(c, label_actions=1, obs=c.misaligned(1, _n, c.F)), _LABEL),
    ("order-obs-begin", "queued", lambda c: raw(c, obs=c.misaligned(1, _n, c.F)), _OBS),
    ("order-flags-begin", "base", lambda c: raw(c, flags=0), _FLAGS),
]
# f32 slots of 70 envs are 16-byte aligned only for an even feature count (tests/refusal_cases.py)
if (N_ENVS * make_tables(WORLDS["base"])[3].n_features * 4) % 16:
    _rows.append(("ring-slot", "begun",
                  lambda c: c.sim.rollout_teach_stream(1, obs=c.t(2, _n, c.F, dtype=torch.float32)), _OBS))
ROWS = [Row("rollout_teach_stream-" + i, _W, h, call, _E, msg) for i, h, call, msg in _rows]
