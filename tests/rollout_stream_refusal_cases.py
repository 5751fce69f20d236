"""What craft_rollout_stream refuses (psketch_amd/csrc/craft_checks_rollout_stream.h), one row per
refusal in the manner of tests/refusal_cases.py, whose handles, Row and check_row these use:
tests/test_rollout_stream_cpu.py runs the table on the CPU variant,
tests/test_gpu_rollout_stream.py on the HIP library.  Both must refuse every row before any work,
with this status and this text, and leave the handle as it was."""
import ctypes

import torch

from psketch_amd import _native as N
from tests.refusal_cases import N_ENVS, Row, make_tables, WORLDS

HANDLES = ("base", "queued", "begun")
_E, _n = N.EINVAL, N_ENVS


def raw(c, flags=N.STEP_AUTORESET, n_ticks=1, ring=1, tick0=0):
    """Straight to the library: the binding always passes CRAFT_STEP_AUTORESET and a ring >= 1."""
    args = N.craft_rollout_stream_args_t()
    args.flags, args.n_ticks, args.ring, args.tick0 = flags, n_ticks, ring, tick0
    return c.L.craft_rollout_stream(c.h, ctypes.byref(args), c.stream())


_BEGIN = "craft_rollout_stream: craft_episode_begin has not put the slots on the queue"
_NEED = "craft_rollout_stream: need n_ticks >= 0, ring >= 1, tick0 >= 0"
_rows = [
    ("rollout_stream-flags0", "craft_rollout_stream", "begun", lambda c: raw(c, flags=0), _E,
     "craft_rollout_stream: flags must be CRAFT_STEP_AUTORESET"),
    ("rollout_stream-flags3", "craft_rollout_stream", "begun", lambda c: raw(c, flags=3), _E,
     "craft_rollout_stream: flags must be CRAFT_STEP_AUTORESET"),
    ("rollout_stream-none", "craft_rollout_stream", "base", lambda c: c.sim.rollout_stream(1), _E, _BEGIN),
    ("rollout_stream-queued", "craft_rollout_stream", "queued", lambda c: c.sim.rollout_stream(1), _E, _BEGIN),
    ("rollout_stream-ticks", "craft_rollout_stream", "begun", lambda c: raw(c, n_ticks=-1), _E, _NEED),
    ("rollout_stream-ring", "craft_rollout_stream", "begun", lambda c: raw(c, ring=0), _E, _NEED),
    ("rollout_stream-tick0", "craft_rollout_stream", "begun", lambda c: c.sim.rollout_stream(1, tick0=-1), _E, _NEED),
    ("rollout_stream-obs", "craft_rollout_stream", "begun",
     lambda c: c.sim.rollout_stream(1, obs=c.misaligned(1, _n, c.F)), _E,
     "craft_rollout_stream: every obs ring slot must be 16-byte aligned"),
]
# f32 slots of 70 envs are 16-byte aligned only for an even feature count (tests/refusal_cases.py)
if (N_ENVS * make_tables(WORLDS["base"])[3].n_features * 4) % 16:
    _rows.append(("rollout_stream-ring-slot", "craft_rollout_stream", "begun",
                  lambda c: c.sim.rollout_stream(1, obs=c.t(2, _n, c.F, dtype=torch.float32)), _E,
                  "craft_rollout_stream: every obs ring slot must be 16-byte aligned"))
ROWS = [Row(*r) for r in _rows]
