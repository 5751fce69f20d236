"""What craft_episode_actions and craft_rollout_replay refuse
(psketch_amd/csrc/craft_checks_rollout_replay.h), one row per refusal in the manner of
tests/refusal_cases.py, whose Ctx, Row and check_row these use: tests/test_rollout_replay_cpu.py
runs the table on the CPU variant, tests/test_gpu_rollout_replay.py on the HIP library.  Both must
refuse every row before any work, with this status and this text, and leave the handle as it was.

Handles: base (no queue), queued (a queue, not begun), begun (begun, no tape) of
tests/refusal_cases.py, and taped: begun with a tape of one STOP per entry."""
import ctypes

import numpy as np
import torch

from psketch_amd import _native as N
from tests.refusal_cases import N_ENVS, QUEUE, Ctx, Row, make_tables, WORLDS

HANDLES = ("base", "queued", "begun", "taped")
_E, _n = N.EINVAL, N_ENVS


def stop_tape(c, count=QUEUE):
    """One STOP per entry, -1 padded."""
    t = np.full((count, c.cfg.max_timesteps), -1, dtype=np.int32)
    t[:, 0] = N.STOP
    return t


def make_replay_handles(device):
    h = {name: Ctx("begun" if name == "taped" else name, device) for name in HANDLES}
    h["taped"].sim.set_episode_actions(torch.as_tensor(stop_tape(h["taped"])))
    return h


def raw(c, flags=N.STEP_AUTORESET, n_ticks=1, ring=1, tick0=0, actions=None):
    """Straight to the library: the binding always passes CRAFT_STEP_AUTORESET, a ring >= 1 and
    no actions."""
    args = N.craft_rollout_replay_args_t()
    r = args.roll
    r.flags, r.n_ticks, r.ring, r.tick0 = flags, n_ticks, ring, tick0
    if actions is not None:
        c._keep = actions
        r.actions = actions.data_ptr()
    return c.L.craft_rollout_replay(c.h, ctypes.byref(args), c.stream())


def install(c, edit=None, count=QUEUE):
    """craft_episode_actions of the all-STOP tape after edit(tape) changed it."""
    t = stop_tape(c, count)
    if edit is not None:
        edit(t)
    return c.sim.set_episode_actions(torch.as_tensor(t))


def _set(e, values):
    """An edit: row e := values (then -1), and a later bad row: the lowest index is named."""
    def edit(t):
        t[e] = -1
        t[e, :len(values)] = values
        t[e + 4, 0] = 9
    return edit


def _bad(e):
    return (f"craft_episode_actions: entry {e} is invalid (1..max_timesteps actions in 0..5 then -1, "
            "ending in its only STOP or max_timesteps long)")


_BEGIN = "craft_rollout_replay: craft_episode_begin has not put the slots on the queue"
_NEED = "craft_rollout_replay: need n_ticks >= 0, ring >= 1, tick0 >= 0"
_FLAGS = "craft_rollout_replay: flags must be CRAFT_STEP_AUTORESET"
_ACTS = "craft_rollout_replay: roll.actions must be NULL (the actions are the tape's)"
_TAPE = "craft_rollout_replay: no actions installed for the current queue (craft_episode_actions)"
_ROWS_MSG = f"craft_episode_actions: need one row per queue entry ({QUEUE}), or NULL and 0 to drop the tape"
_rows = [
    # ---- craft_episode_actions, on a handle with a tape (which must stay in force) and without
    ("actions-six", "craft_episode_actions", "taped", lambda c: install(c, _set(7, [0, 6, N.STOP])), _E, _bad(7)),
    ("actions-minus2", "craft_episode_actions", "taped", lambda c: install(c, _set(3, [0, -2, N.STOP])), _E, _bad(3)),
    ("actions-early-stop", "craft_episode_actions", "taped",
     lambda c: install(c, _set(5, [0, N.STOP, 1, N.STOP])), _E, _bad(5)),
    ("actions-short", "craft_episode_actions", "taped", lambda c: install(c, _set(0, [0, 1])), _E, _bad(0)),
    ("actions-empty", "craft_episode_actions", "taped", lambda c: install(c, _set(11, [])), _E, _bad(11)),
    ("actions-gap", "craft_episode_actions", "taped", lambda c: install(c, _set(2, [0, -1, N.STOP])), _E, _bad(2)),
    ("actions-short-begun", "craft_episode_actions", "begun", lambda c: install(c, _set(1, [2])), _E, _bad(1)),
    ("actions-count", "craft_episode_actions", "taped", lambda c: install(c, count=QUEUE - 1), _E, _ROWS_MSG),
    ("actions-count-more", "craft_episode_actions", "queued", lambda c: install(c, count=QUEUE + 1), _E, _ROWS_MSG),
    ("actions-null-count", "craft_episode_actions", "taped",
     lambda c: c.L.craft_episode_actions(c.h, None, QUEUE), _E, _ROWS_MSG),
    ("actions-no-queue", "craft_episode_actions", "base", lambda c: install(c), _E,
     "craft_episode_actions: no episode queue installed (craft_episode_queue)"),
    ("actions-no-queue-drop", "craft_episode_actions", "base", lambda c: c.sim.set_episode_actions(None), _E,
     "craft_episode_actions: no episode queue installed (craft_episode_queue)"),
    # ---- craft_rollout_replay: craft_rollout_stream's refusals first, in its order (each with
    # actions set and, on begun, no tape: the later tests must not be reached), then its own two
    ("replay-flags0", "craft_rollout_replay", "begun", lambda c: raw(c, flags=0, actions=c.t(_n)), _E, _FLAGS),
    ("replay-flags3", "craft_rollout_replay", "taped", lambda c: raw(c, flags=3, n_ticks=-1), _E, _FLAGS),
    ("replay-ticks", "craft_rollout_replay", "begun", lambda c: raw(c, n_ticks=-1, actions=c.t(_n)), _E, _NEED),
    ("replay-ring", "craft_rollout_replay", "taped", lambda c: raw(c, ring=0), _E, _NEED),
    ("replay-tick0", "craft_rollout_replay", "taped", lambda c: c.sim.rollout_replay(1, tick0=-1), _E, _NEED),
    ("replay-obs", "craft_rollout_replay", "begun",
     lambda c: c.sim.rollout_replay(1, obs=c.misaligned(1, _n, c.F)), _E,
     "craft_rollout_replay: every obs ring slot must be 16-byte aligned"),
    ("replay-none", "craft_rollout_replay", "base", lambda c: raw(c, actions=c.t(_n)), _E, _BEGIN),
    ("replay-queued", "craft_rollout_replay", "queued", lambda c: c.sim.rollout_replay(1), _E, _BEGIN),
    ("replay-actions", "craft_rollout_replay", "taped", lambda c: raw(c, actions=c.t(_n)), _E, _ACTS),
    ("replay-actions-no-tape", "craft_rollout_replay", "begun", lambda c: raw(c, actions=c.t(_n)), _E, _ACTS),
    ("replay-no-tape", "craft_rollout_replay", "begun", lambda c: c.sim.rollout_replay(1), _E, _TAPE),
    ("replay-no-tape-no-ticks", "craft_rollout_replay", "begun", lambda c: c.sim.rollout_replay(0), _E, _TAPE),
]
# f32 slots of 70 envs are 16-byte aligned only for an even feature count (tests/refusal_cases.py)
if (N_ENVS * make_tables(WORLDS["base"])[3].n_features * 4) % 16:
    _rows.append(("replay-ring-slot", "craft_rollout_replay", "taped",
                  lambda c: c.sim.rollout_replay(1, obs=c.t(2, _n, c.F, dtype=torch.float32)), _E,
                  "craft_rollout_replay: every obs ring slot must be 16-byte aligned"))
ROWS = [Row(*r) for r in _rows]
assert len({r.id for r in ROWS}) == len(ROWS)


def check_tape_survives_refusals(c):
    """After every refused install on the taped handle, its all-STOP tape still drives a launch:
    one tick ends every slot's episode."""
    n = c.n
    end = c.t(1, n, fill=-1)
    nxt = c.t(1, n, fill=-7)
    before = int(c.sim.stats()[1])
    c.sim.rollout_replay(1, episode_end=end, action_next=nxt)
    c.sim.check()
    assert (end.cpu().numpy() >= 0).all()
    assert int(c.sim.stats()[1]) == before + n
    assert (nxt.cpu().numpy() == N.STOP).all()           # the next entries' rows are STOPs too


def check_queue_drops_tape(c):
    """A tape, then craft_episode_queue again: the tape is gone, and stays gone after
    craft_episode_begin; dropping it by hand refuses the same way."""
    sim = c.sim
    sim.set_episode_actions(torch.as_tensor(stop_tape(c)))
    sim.rollout_replay(1)
    sim.set_episode_queue(torch.as_tensor(c.queue))
    sim.begin_episodes()
    for again in (False, True):
        try:
            sim.rollout_replay(1)
            raise AssertionError("rollout_replay ran without a tape")
        except N.CraftError as e:
            assert e.status == N.EINVAL
            assert c.L.craft_sim_last_error(c.h).decode() == _TAPE
        if not again:
            sim.set_episode_actions(torch.as_tensor(stop_tape(c)))
            sim.rollout_replay(1)
            sim.set_episode_actions(None)
    sim.check()
