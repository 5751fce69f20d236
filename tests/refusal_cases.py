"""One row per refusal of the shared argument checks (psketch_amd/csrc/craft_checks.h): the entry
point, the bad call, the status and the full craft_sim_last_error text.  tests/test_refusals.py
runs the table on the CPU variant, tests/test_gpu_refusals.py on the HIP library and the CPU
variant side by side.  Both libraries must refuse every row before any work, with this status and
this text, and leave the handle as it was.

The bad call goes through the binding where the binding lets the argument through, else straight
to the library (c.L) with tiny tensors.  The texts were copied from the libraries' sources as
they stood before the checks moved into the shared header.

Handles (Ctx), all tiny: 70 envs (not a multiple of any tile), a 4-row pool.
  base    12x12, 3x3 window, reset, no episode queue
  w5      12x12, 5x5 window, reset: the knob rows (at 5x5 craft_sim_rollout_shape shows tile_envs)
  queued  as base, with an episode queue installed but not begun
  begun   as queued, begun without wrap
  big     16x16 (4*W*H = 1024 > 1000), reset, its queue begun: the six BFS-queue refusals
  k32w7   15x16, 7x7 window, the 32 kinds of tests/golden/recipes.limits.yaml, reset: the tile that
          does not fit a workgroup's LDS
"""
import ctypes
import os
from collections import namedtuple

import numpy as np
import torch

from psketch_amd import CraftSim, sample_scenarios, synthetic_specs
from psketch_amd import _native as N
from tests.helpers import make_tables, rect_world

N_ENVS, POOL = 70, 4
QUEUE = 3 * N_ENVS + 17
WORLDS = {"base": "craft_medium_12x12", "w5": "craft_medium_12x12_w5", "queued": "craft_medium_12x12",
          "begun": "craft_medium_12x12", "big": rect_world(16, 16, 3), "k32w7": rect_world(15, 16, 7)}
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COOKBOOKS = {"k32w7": dict(recipes=os.path.join(_GOLDEN, "recipes.limits.yaml"),
                           hints=os.path.join(_GOLDEN, "hints.limits.yaml"))}

Row = namedtuple("Row", "id entry handle call status message")


class Ctx:
    """One handle with what the rows' calls need: its pool, reset specs, queue specs and a few
    tensors on its device."""

    def __init__(self, name, device):
        world = WORLDS[name]
        kw = COOKBOOKS.get(name, {})
        params, cb, tm, cfg = make_tables(world, **kw)
        W, H = params["WIDTH"], params["HEIGHT"]
        self.name, self.cfg = name, cfg
        self.pool, _, _ = sample_scenarios(params, cb, 123, POOL)
        tasks = [t.id for t in tm.dataset_tasks()]
        self.specs = synthetic_specs(self.pool, W, H, N_ENVS, 0, seed=7, task_ids=tasks)
        self.queue = np.ascontiguousarray(
            np.stack(synthetic_specs(self.pool, W, H, QUEUE, 0, seed=9, task_ids=tasks), 1).astype(np.int32))
        self.sim = sim = CraftSim(world, n_envs=N_ENVS, device=device, pool_capacity=POOL, **kw)
        sim.load_pool(self.pool)
        sim.reset(*self.specs)
        if name in ("queued", "begun", "big"):
            sim.set_episode_queue(torch.as_tensor(self.queue))
        if name in ("begun", "big"):
            sim.begin_episodes()
        self.L, self.h, self.n, self.F = sim._L, sim._h, N_ENVS, sim.n_features

    def stream(self):
        return self.sim._stream()

    def t(self, *shape, dtype=torch.int32, fill=0):
        return torch.full(shape, fill, dtype=dtype, device=self.sim.device)

    def misaligned(self, *shape):
        """An observation buffer of the handle's format that starts 4 bytes past a 16-byte
        boundary (contiguous, the right shape: the binding passes it on)."""
        numel = int(np.prod(shape))
        base = torch.zeros(numel + 16, dtype=self.sim.obs_dtype, device=self.sim.device)
        assert base.data_ptr() % 16 == 0
        return base[1:1 + numel].view(*shape)

    def generate(self, first=0, count=1, boundary=None, prims=None, ws=None, n_per=None):
        """craft_pool_generate with the cookbook's arguments but for the ones given."""
        from psketch_amd.cookbook import generator_primitives
        sim = self.sim
        boundary = sim.cookbook.index["boundary"] if boundary is None else boundary
        prims = np.ascontiguousarray(generator_primitives(sim.cookbook) if prims is None else prims, dtype=np.int32)
        ws = np.asarray([sim.cookbook.index["workshop%d" % i] for i in range(3)] if ws is None else ws,
                        dtype=np.int32)
        n_per = sim.params["N_PRIMITIVES"] if n_per is None else n_per
        return self.L.craft_pool_generate(self.h, 1, 0, first, count, boundary, prims.ctypes.data, len(prims),
                                          n_per, ws.ctypes.data, len(ws), None, self.stream())

    def distances(self, ok=True):
        n = self.n
        a = [self.t(n), self.t(n, dtype=torch.int8), self.t(2, n), 2, self.t(n), self.t(n, dtype=torch.uint8),
             self.t(n), self.t(2)]
        if not ok:
            a[0] = None
        self._keep = a
        ptr = [x if isinstance(x, int) or x is None else x.data_ptr() for x in a]
        return self.L.craft_rollout_distances(self.h, *ptr, self.stream())

    def stream_raw(self, flags):
        args = N.craft_stream_step_args_t()
        args.step.flags = flags
        return self.L.craft_step_stream(self.h, ctypes.byref(args), self.stream())

    def bad_queue(self, index):
        q = self.queue.copy()
        q[index, 0] = POOL                   # a scenario past the pool
        q[index + 4, 4] = -1                 # and a later bad task: the lowest index is named
        return torch.as_tensor(q)


def make_handles(device, names=tuple(WORLDS)):
    return {name: Ctx(name, device) for name in names}


def _bfs(who):
    return who + ": 4*W*H > 1000 overflows the reference's BFS queue (teachers/base.py:42)"


_E, _R = N.EINVAL, N.ERANGE
_n = N_ENVS
_rows = [
    # ---- the knobs
    ("tune-tile48", "craft_sim_tune", "w5", lambda c: c.sim.tune(48, 0, 0), _E,
     "craft_sim_tune: tile_envs must be 16, 32 or 64"),
    ("tune-tile-1", "craft_sim_tune", "w5", lambda c: c.sim.tune(-1, 0, 0), _E,
     "craft_sim_tune: tile_envs must be 16, 32 or 64"),
    ("tune-tile64-k32w7", "craft_sim_tune", "k32w7", lambda c: c.sim.tune(64, 0, 2), _E,
     "craft_sim_tune: a tile of tile_envs envs does not fit a workgroup's 160 KiB of LDS with this window and kind "
     "count"),
    ("tune-resident2", "craft_sim_tune", "w5", lambda c: c.sim.tune(16, 2, 1), _E,
     "craft_sim_tune: max_resident_per_cu must be 0 or 3..32"),
    ("tune-resident33", "craft_sim_tune", "w5", lambda c: c.sim.tune(16, 33, 1), _E,
     "craft_sim_tune: max_resident_per_cu must be 0 or 3..32"),
    ("tune-store3", "craft_sim_tune", "w5", lambda c: c.sim.tune(16, 4, 3), _E,
     "craft_sim_tune: obs_store must be 0 (write-back), 1 (nontemporal) or 2 (write-through)"),
    ("tune_teach-kernel", "craft_sim_tune_teach", "w5", lambda c: c.sim.tune_teach(3, 1, 2), _E,
     "craft_sim_tune_teach: kernel must be 0 (auto), 1 (one-tile) or 2 (two-tile)"),
    ("tune_teach-lanes", "craft_sim_tune_teach", "w5", lambda c: c.sim.tune_teach(1, 3, 2), _E,
     "craft_sim_tune_teach: lanes must be 0 (default), 1, 2 or 4"),
    ("tune_teach-table", "craft_sim_tune_teach", "w5", lambda c: c.sim.tune_teach(1, 1, 3), _E,
     "craft_sim_tune_teach: table must be 0 (auto), 1 (always) or 2 (never)"),
    ("tune_host-neg", "craft_sim_tune_host", "w5", lambda c: c.sim.tune_host(-1), _E,
     "craft_sim_tune_host: threads must be 0 (the machine's) or 1..1024"),
    ("tune_host-big", "craft_sim_tune_host", "w5", lambda c: c.sim.tune_host(1025), _E,
     "craft_sim_tune_host: threads must be 0 (the machine's) or 1..1024"),
    ("tune_rollout-chunk", "craft_sim_tune_rollout", "w5", lambda c: c.sim.tune_rollout(4097, 128), _E,
     "craft_sim_tune_rollout: chunk_ticks must be -1..4096"),
    ("tune_rollout-threads", "craft_sim_tune_rollout", "w5", lambda c: c.sim.tune_rollout(4, 64), _E,
     "craft_sim_tune_rollout: threads must be 0, 128, 256, 320, 384 or 512"),
    ("obs_format", "craft_sim_set_obs_format", "w5", lambda c: c.L.craft_sim_set_obs_format(c.h, 3), _E,
     "craft_sim_set_obs_format: format must be 0 (fp32), 1 (bf16) or 2 (u8)"),
    # ---- the pool
    ("pool_load-null", "craft_pool_load", "base", lambda c: c.L.craft_pool_load(c.h, None, 0, 1), _E,
     "craft_pool_load: bad argument"),
    ("pool_load-first", "craft_pool_load", "base", lambda c: c.sim.load_pool(c.pool[:1], first=-1), _E,
     "craft_pool_load: bad argument"),
    ("pool_load-capacity", "craft_pool_load", "base", lambda c: c.sim.load_pool(c.pool[:2], first=POOL - 1), _R,
     "craft_pool_load: beyond pool capacity"),
    ("pool_generate-count", "craft_pool_generate", "base", lambda c: c.sim.generate_pool(-1), _E,
     "craft_pool_generate: bad argument"),
    ("pool_generate-nprims", "craft_pool_generate", "base", lambda c: c.generate(prims=[1] * 9), _E,
     "craft_pool_generate: bad argument"),
    ("pool_generate-capacity", "craft_pool_generate", "base", lambda c: c.sim.generate_pool(2, first=POOL - 1), _R,
     "craft_pool_generate: beyond pool capacity"),
    ("pool_generate-boundary", "craft_pool_generate", "base", lambda c: c.generate(boundary=0), _E,
     "craft_pool_generate: bad boundary kind"),
    ("pool_generate-primitive", "craft_pool_generate", "base",
     lambda c: c.generate(prims=[1, c.sim.n_kinds]), _E, "craft_pool_generate: bad primitive kind"),
    ("pool_generate-workshop", "craft_pool_generate", "base", lambda c: c.generate(ws=[1, 2, -1]), _E,
     "craft_pool_generate: bad workshop kind"),
    ("pool_generate-crowded", "craft_pool_generate", "base", lambda c: c.generate(n_per=50), _E,
     "craft_pool_generate: more objects than interior cells"),
    # ---- reset and the ticks
    ("reset-null", "craft_reset", "base",
     lambda c: c.L.craft_reset(c.h, None, *[c.t(_n).data_ptr()] * 4, None, c.stream()), _E,
     "craft_reset: null input"),
    ("reset-obs", "craft_reset", "base", lambda c: c.sim.reset(*c.specs, obs=c.misaligned(_n, c.F)), _E,
     "craft_reset: obs must be 16-byte aligned"),
    ("step-obs", "craft_step", "base", lambda c: c.sim.step(obs=c.misaligned(_n, c.F)), _E,
     "craft_step: obs must be 16-byte aligned"),
    ("step_ex-obs", "craft_step_ex", "base",
     lambda c: c.sim.step(obs=c.misaligned(_n, c.F), action_record=c.t(_n)), _E,
     "craft_step: obs must be 16-byte aligned"),
    ("step_ex-clone", "craft_step_ex", "base",
     lambda c: c.sim.step(behavior_clone=c.t(_n, dtype=torch.uint8, fill=1)), _E,
     "craft_step_ex: behavior_clone needs ref_actions"),
    ("step_teach-obs", "craft_step_teach", "base",
     lambda c: c.sim.step(obs=c.misaligned(_n, c.F), labels=c.t(_n)), _E,
     "craft_step: obs must be 16-byte aligned"),
    ("step_teach-clone", "craft_step_teach", "base",
     lambda c: c.sim.step(behavior_clone=c.t(_n, dtype=torch.uint8, fill=1), labels=c.t(_n)), _E,
     "craft_step_ex: behavior_clone needs ref_actions"),
    ("step_teach-bfs", "craft_step_teach", "big", lambda c: c.sim.step(labels=c.t(_n)), _E,
     _bfs("craft_step_teach")),
    ("step_lang-flags", "craft_step_lang", "base", lambda c: c.sim.step_lang(flags=1), _E,
     "craft_step_lang: flags must be 0 (no auto-reset in this protocol)"),
    ("step_lang-alt", "craft_step_lang", "base",
     lambda c: c.sim.step_lang(use_alt=c.t(_n, dtype=torch.uint8, fill=1)), _E,
     "craft_step_lang: use_alt needs alt_actions"),
    ("step_lang-obs", "craft_step_lang", "base", lambda c: c.sim.step_lang(obs=c.misaligned(_n, c.F)), _E,
     "craft_step_lang: obs must be 16-byte aligned"),
    ("step_lang-bfs", "craft_step_lang", "big", lambda c: c.sim.step_lang(labels=c.t(_n)), _E,
     _bfs("craft_step_lang")),
    # ---- the episode queue
    ("episode_queue-null", "craft_episode_queue", "queued", lambda c: c.L.craft_episode_queue(c.h, None, 5), _E,
     "craft_episode_queue: specs must hold 1 .. 2^31 - 1 entries"),
    ("episode_queue-empty", "craft_episode_queue", "queued",
     lambda c: c.L.craft_episode_queue(c.h, c.t(5).data_ptr(), 0), _E,
     "craft_episode_queue: specs must hold 1 .. 2^31 - 1 entries"),
    ("episode_queue-huge", "craft_episode_queue", "queued",
     lambda c: c.L.craft_episode_queue(c.h, c.t(5).data_ptr(), 2 ** 31), _E,
     "craft_episode_queue: specs must hold 1 .. 2^31 - 1 entries"),
    ("episode_queue-entry", "craft_episode_queue", "queued", lambda c: c.sim.set_episode_queue(c.bad_queue(5)), _E,
     "craft_episode_queue: entry 5 is invalid (scenario, position, direction or task out of range)"),
    ("episode_queue-entry-begun", "craft_episode_queue", "begun",
     lambda c: c.sim.set_episode_queue(c.bad_queue(0)), _E,
     "craft_episode_queue: entry 0 is invalid (scenario, position, direction or task out of range)"),
    ("episode_begin-none", "craft_episode_begin", "base", lambda c: c.sim.begin_episodes(), _E,
     "craft_episode_begin: no episode queue installed (craft_episode_queue)"),
    ("episode_begin-stride", "craft_episode_begin", "queued", lambda c: c.sim.begin_episodes(stride=0), _E,
     "craft_episode_begin: stride must be >= 1"),
    ("episode_begin-first", "craft_episode_begin", "queued", lambda c: c.sim.begin_episodes(first=-1), _E,
     "craft_episode_begin: first must be >= 0"),
    ("episode_begin-flag", "craft_episode_begin", "queued",
     lambda c: c.L.craft_episode_begin(c.h, 0, _n, 2, None, c.stream()), _E,
     "craft_episode_begin: unknown flag"),
    ("episode_begin-obs", "craft_episode_begin", "queued",
     lambda c: c.sim.begin_episodes(obs=c.misaligned(_n, c.F)), _E,
     "craft_episode_begin: obs must be 16-byte aligned"),
    ("episode_begin-range", "craft_episode_begin", "queued",
     lambda c: c.sim.begin_episodes(first=2 ** 63 - 1, wrap=True), _E,
     "craft_episode_begin: first is out of range"),
    ("episode_begin-past", "craft_episode_begin", "queued",
     lambda c: c.sim.begin_episodes(first=QUEUE - _n + 1), _E,
     f"craft_episode_begin: slot {_n - 1} would start past the end of the queue ({QUEUE} entries)"),
    ("episode_begin-past-begun", "craft_episode_begin", "begun",
     lambda c: c.sim.begin_episodes(first=QUEUE + 3), _E,
     f"craft_episode_begin: slot 0 would start past the end of the queue ({QUEUE} entries)"),
    ("step_stream-flags0", "craft_step_stream", "begun", lambda c: c.stream_raw(0), _E,
     "craft_step_stream: step.flags must be CRAFT_STEP_AUTORESET"),
    ("step_stream-flags3", "craft_step_stream", "begun", lambda c: c.stream_raw(3), _E,
     "craft_step_stream: step.flags must be CRAFT_STEP_AUTORESET"),
    ("step_stream-none", "craft_step_stream", "base", lambda c: c.sim.step_stream(), _E,
     "craft_step_stream: craft_episode_begin has not put the slots on the queue"),
    ("step_stream-queued", "craft_step_stream", "queued", lambda c: c.sim.step_stream(), _E,
     "craft_step_stream: craft_episode_begin has not put the slots on the queue"),
    ("step_stream-bfs", "craft_step_stream", "big", lambda c: c.sim.step_stream(labels=c.t(_n)), _E,
     _bfs("craft_step_stream")),
    ("step_stream-obs", "craft_step_stream", "begun", lambda c: c.sim.step_stream(obs=c.misaligned(_n, c.F)), _E,
     "craft_step: obs must be 16-byte aligned"),
    ("step_stream-clone", "craft_step_stream", "begun",
     lambda c: c.sim.step_stream(behavior_clone=c.t(_n, dtype=torch.uint8, fill=1)), _E,
     "craft_step_ex: behavior_clone needs ref_actions"),
    # ---- the multi-tick launches
    ("rollout-ticks", "craft_rollout", "base",
     lambda c: c.L.craft_rollout(c.h, None, 0, 0, -1, 1, None, 1, None, None, None, c.stream()), _E,
     "craft_rollout: need n_ticks >= 0, ring >= 1, tick0 >= 0"),
    ("rollout-ring", "craft_rollout", "base",
     lambda c: c.L.craft_rollout(c.h, None, 0, 0, 1, 1, None, 0, None, None, None, c.stream()), _E,
     "craft_rollout: need n_ticks >= 0, ring >= 1, tick0 >= 0"),
    ("rollout-tick0", "craft_rollout", "base", lambda c: c.sim.rollout(1, tick0=-1), _E,
     "craft_rollout: need n_ticks >= 0, ring >= 1, tick0 >= 0"),
    ("rollout-obs", "craft_rollout", "base", lambda c: c.sim.rollout(1, obs=c.misaligned(1, _n, c.F)), _E,
     "craft_rollout: every obs ring slot must be 16-byte aligned"),
    ("rollout_teach-ticks", "craft_rollout_teach", "base", lambda c: c.sim.rollout_teach(1, tick0=-1), _E,
     "craft_rollout_teach: need n_ticks >= 0, ring >= 1, tick0 >= 0"),
    ("rollout_teach-bfs", "craft_rollout_teach", "big", lambda c: c.sim.rollout_teach(1, labels=c.t(1, _n)), _E,
     _bfs("craft_rollout_teach")),
    ("rollout_teach-label_actions", "craft_rollout_teach", "base",
     lambda c: c.sim.rollout_teach(1, label_actions=True), _E,
     "craft_rollout_teach: label_actions / behavior_clone need label_in"),
    ("rollout_teach-clone", "craft_rollout_teach", "base",
     lambda c: c.sim.rollout_teach(1, behavior_clone=c.t(_n, dtype=torch.uint8, fill=1)), _E,
     "craft_rollout_teach: label_actions / behavior_clone need label_in"),
    ("rollout_teach-obs", "craft_rollout_teach", "base",
     lambda c: c.sim.rollout_teach(1, obs=c.misaligned(1, _n, c.F)), _E,
     "craft_rollout_teach: every obs ring slot must be 16-byte aligned"),
    ("rollout_distances-null", "craft_rollout_distances", "base", lambda c: c.distances(ok=False), _E,
     "craft_rollout_distances: bad argument"),
    ("rollout_distances-bfs", "craft_rollout_distances", "big", lambda c: c.distances(), _E,
     _bfs("craft_rollout_distances")),
    # ---- the slot-list calls
    ("transition-null", "craft_transition", "base",
     lambda c: c.L.craft_transition(c.h, None, None, None, 3, None, c.stream()), _E,
     "craft_transition: bad argument"),
    ("transition-neg", "craft_transition", "base",
     lambda c: c.L.craft_transition(c.h, None, None, c.t(3).data_ptr(), -1, None, c.stream()), _E,
     "craft_transition: bad argument"),
    ("transition-n", "craft_transition", "base", lambda c: c.sim.transition(c.t(_n + 1)), _R,
     "craft_transition: n > n_envs"),
    ("observe-neg", "craft_observe", "base", lambda c: c.sim.observe(n=-1), _E, "craft_observe: bad argument"),
    ("observe-n", "craft_observe", "base", lambda c: c.sim.observe(n=_n + 1), _R, "craft_observe: n > n_envs"),
    ("observe-obs", "craft_observe", "base", lambda c: c.sim.observe(obs=c.misaligned(_n, c.F)), _E,
     "craft_observe: obs must be 16-byte aligned"),
    ("teacher-null", "craft_teacher", "base",
     lambda c: c.L.craft_teacher(c.h, None, 3, None, None, None, c.stream()), _E, "craft_teacher: bad argument"),
    ("teacher-n", "craft_teacher", "base", lambda c: c.sim.teacher(n=_n + 1), _R, "craft_teacher: n > n_envs"),
    ("teacher-bfs", "craft_teacher", "big", lambda c: c.sim.teacher(), _E, _bfs("craft_teacher")),
    ("get_state-neg", "craft_get_state", "base",
     lambda c: c.L.craft_get_state(c.h, None, -1, None, None, None, None, c.stream()), _E,
     "craft_get_state: bad argument"),
    ("get_state-n", "craft_get_state", "base", lambda c: c.sim.get_state(n=_n + 1), _R,
     "craft_get_state: n > n_envs"),
    ("set_state-null", "craft_set_state", "base",
     lambda c: c.L.craft_set_state(c.h, None, 3, None, None, None, c.stream()), _E,
     "craft_set_state: bad argument"),
    ("set_state-n", "craft_set_state", "base", lambda c: c.sim.set_state(c.t(_n + 1, 5), c.t(_n + 1, 4)), _R,
     "craft_set_state: n > n_envs"),
]
# f32 slots of 70 envs are 16-byte aligned only for an even feature count: with an odd one, a ring
# of two slots on an aligned base is refused as well
if (N_ENVS * make_tables(WORLDS["base"])[3].n_features * 4) % 16:
    _rows += [
        ("rollout-ring-slot", "craft_rollout", "base",
         lambda c: c.sim.rollout(1, obs=c.t(2, _n, c.F, dtype=torch.float32)), _E,
         "craft_rollout: every obs ring slot must be 16-byte aligned"),
        ("rollout_teach-ring-slot", "craft_rollout_teach", "base",
         lambda c: c.sim.rollout_teach(1, obs=c.t(2, _n, c.F, dtype=torch.float32)), _E,
         "craft_rollout_teach: every obs ring slot must be 16-byte aligned"),
    ]
ROWS = [Row(*r) for r in _rows]
assert len({r.id for r in ROWS}) == len(ROWS)


def refuse(c, row):
    """Makes the row's call on c; returns (status, craft_sim_last_error's text)."""
    try:
        status = row.call(c)
    except N.CraftError as e:
        status = e.status
    return status, c.L.craft_sim_last_error(c.h).decode()


def snapshot(c):
    """What a refused call must leave as it was: the shapes the knobs resolve to, every slot's
    state, the episode counters."""
    sim = c.sim
    st = sim.get_state()
    return {"step_shape": (sim.step_shape(False), sim.step_shape(True)), "rollout_shape": sim.rollout_shape(),
            "tile_shape": sim.tile_shape(), "stats": sim.stats().cpu().tolist(),
            **{"state." + k: v.cpu().numpy() for k, v in st.items()}}


def assert_unchanged(before, after, what):
    assert before.keys() == after.keys()
    for k in before:
        if isinstance(before[k], np.ndarray):
            np.testing.assert_array_equal(after[k], before[k], err_msg=f"{what}: {k} changed")
        else:
            assert after[k] == before[k], f"{what}: {k} changed from {before[k]} to {after[k]}"


def check_row(c, row):
    """The row on handle c: refused with the table's status and text, nothing changed, nothing
    latched."""
    before = snapshot(c)
    status, msg = refuse(c, row)
    assert (status, msg) == (row.status, row.message), row.id
    assert_unchanged(before, snapshot(c), row.id)
    c.sim.check()


def check_valid_tick(c, oracle_mod):
    """One tick of c (reset to c.specs, never stepped) against the oracle's."""
    sim, n = c.sim, c.n
    o = oracle_mod.Oracle(c.cfg, c.pool)
    envs = o.init_envs(*c.specs)
    obs = sim.empty_obs()
    rew, done, succ = c.t(n, dtype=torch.float32), c.t(n, dtype=torch.uint8), c.t(n, dtype=torch.int8)
    sim.step(seed=5, tick=0, obs=obs, reward=rew, done=done, success=succ)
    rc, oobs, orew, odone, osucc = o.batch_tick(envs, 0, None, 5, 0, True)
    assert rc == 0
    np.testing.assert_array_equal(obs.cpu().numpy(), oobs)
    np.testing.assert_array_equal(rew.cpu().numpy(), orew)
    np.testing.assert_array_equal(done.cpu().numpy(), odone)
    np.testing.assert_array_equal(succ.cpu().numpy(), osucc)
    sim.check()
