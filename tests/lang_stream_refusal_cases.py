"""One row per refusal of craft_step_lang_stream's shared argument check
(psketch_amd/csrc/craft_checks_lang_stream.h), in the manner of tests/refusal_cases.py, whose
handles, Row and check_row these rows use: the bad call, the status and the full
craft_sim_last_error text.  tests/test_lang_stream_cpu.py runs the table on the CPU variant,
tests/test_gpu_step_lang_stream.py on the HIP library."""
import ctypes

import torch

from psketch_amd import _native as N
from tests.refusal_cases import N_ENVS, Row, _bfs

HANDLES = ("base", "queued", "begun", "big")
_E, _n = N.EINVAL, N_ENVS


def _raw(c, flags):
    args = N.craft_lang_stream_step_args_t()
    args.step.flags = flags
    return c.L.craft_step_lang_stream(c.h, ctypes.byref(args), c.stream())


_NOT_BEGUN = "craft_step_lang_stream: craft_episode_begin has not put the slots on the queue"
ROWS = [Row(*r) for r in (
    ("step_lang_stream-flags1", "craft_step_lang_stream", "begun", lambda c: c.sim.step_lang_stream(flags=1), _E,
     "craft_step_lang_stream: step.flags must be 0 (the queue is the restart)"),
    ("step_lang_stream-flags2", "craft_step_lang_stream", "begun", lambda c: _raw(c, 2), _E,
     "craft_step_lang_stream: step.flags must be 0 (the queue is the restart)"),
    ("step_lang_stream-alt", "craft_step_lang_stream", "begun",
     lambda c: c.sim.step_lang_stream(use_alt=c.t(_n, dtype=torch.uint8, fill=1)), _E,
     "craft_step_lang_stream: use_alt needs alt_actions"),
    ("step_lang_stream-obs", "craft_step_lang_stream", "begun",
     lambda c: c.sim.step_lang_stream(obs=c.misaligned(_n, c.F)), _E,
     "craft_step_lang_stream: obs must be 16-byte aligned"),
    ("step_lang_stream-none", "craft_step_lang_stream", "base", lambda c: c.sim.step_lang_stream(), _E, _NOT_BEGUN),
    ("step_lang_stream-queued", "craft_step_lang_stream", "queued", lambda c: c.sim.step_lang_stream(), _E,
     _NOT_BEGUN),
    ("step_lang_stream-bfs", "craft_step_lang_stream", "big", lambda c: c.sim.step_lang_stream(labels=c.t(_n)), _E,
     _bfs("craft_step_lang_stream")),
)]
assert len({r.id for r in ROWS}) == len(ROWS)
