"""Shared by tests/test_cookbook_limits.py and tests/test_gpu_cookbook_limits.py: the cookbooks of
tests/golden/recipes.<name>.yaml + hints.<name>.yaml (up to the ABI's 32 kinds, 16 recipes of 4
ingredients, 64 tasks of 4 subtasks), their pools and specs in the layout of tests/rect_cases.py
(whose make_sim and runners take these cases), and the conditions a run asserts it has exercised.
Every condition is computed from the oracle's side or from the inputs, never from the simulator
under test."""
import os
from types import SimpleNamespace as NS

import numpy as np

from psketch_amd import _native as N
from psketch_amd import synthetic_specs
from psketch_amd.cookbook import generator_primitives
from tests.helpers import make_tables, rect_world
from tests.rect_cases import mixed_actions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COOKBOOKS = ("limits", "k32compact", "even", "tiny")
KINDS = {"limits": 32, "k32compact": 32, "even": 22, "tiny": 12}
# tag -> (W, H, window, N_PRIMITIVES); 15x16 is the largest world the teacher takes
WORLDS = {"w3": (12, 12, 3, 2), "w5": (10, 10, 5, 1), "w7": (15, 16, 7, 2)}
# the world of each cookbook's part of tests/golden/cookbook_limits.npz (make_golden.py COOKBOOKS)
FIXTURE_WORLD = {"limits": "w3", "k32compact": "w5", "even": "w7", "tiny": "w3"}
T_MAX = 12                                      # max_timesteps: episodes end and restart within a run


def yaml_paths(name):
    return dict(recipes=os.path.join(GOLDEN, f"recipes.{name}.yaml"), hints=os.path.join(GOLDEN, f"hints.{name}.yaml"))


def cookbook_world(world):
    return rect_world(*WORLDS[world])


def cookbook_tables(name, world="w3", max_timesteps=T_MAX):
    return make_tables(cookbook_world(world), max_timesteps, **yaml_paths(name))


def table_slots(cfg):
    """kind -> teacher-table slot, as include/craft.h states it: the kinds go[] and get[] tasks
    target, in task order, take the slots 0..14; a later one has none (absent here)."""
    slots = {}
    for t in range(cfg.n_tasks):
        tk = cfg.task[t]
        if tk.goal in (N.GOAL_GO, N.GOAL_GET) and tk.arg_kind > 0 and tk.arg_kind not in slots:
            slots[tk.arg_kind] = len(slots)
    return {k: s for k, s in slots.items() if s < 15}, sorted(k for k, s in slots.items() if s >= 15)


def n_predicates(task):
    """Distinct satisfies() predicates of the task's hint tree (get/make X: inventory; go X: the
    facing cell): more than 8 and the kernels walk the hints instead of reading the leaf table."""
    keys, stack = set(), [task]
    while stack:
        t = stack.pop()
        if t.goal_name in ("get", "make"):
            keys.add(("inv", t.goal_arg))
        elif t.goal_name == "go":
            keys.add(("face", t.goal_arg))
        stack.extend(t.subtasks or [])
    return len(keys)


def hint_leaf(o, env, task):
    """teachers/base.py find_incomplete_subtask over the oracle's satisfies: the leaf task the
    teacher acts on, None where the task is satisfied (or the reference raises)."""
    if o.satisfies(env, task.id) == 1:
        return None
    if task.subtasks is None:
        return task
    for s in task.subtasks[:-1]:
        leaf = hint_leaf(o, env, s)
        if leaf is not None:
            return leaf
    return hint_leaf(o, env, task.subtasks[-1])


def _ring(W, H, cb):
    g = np.zeros((W, H), dtype=np.uint8)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = cb.index["boundary"]
    return g


def hand_rows(name, W, H, cb):
    """Hand-built pool rows with their start pose and task, [(grid, x, y, dir, task name)]: what the
    generated scenarios never hold, within a few ticks of the start pose at the world's centre
    (x, y), facing DOWN.  limits: the four ingredients of lamp around the pose and workshop2 two
    cells below (the teacher of make[lamp], a hint tree of 10 predicates that starts at glass, a
    kind without a table slot, crafts it in 10 ticks); stick, coal, flax and workshop1 around it
    (make[torch], 3 ingredients, 8 ticks); crown, kind 31 and the table's slot 14, beside it and
    farther off (get[crown]); glass, no slot, four cells off (get[glass]); crown in the cell the
    pose faces (make[crown]: a random policy grabs it too).  k32compact: ladder, kind 31, beside
    the pose.  Every cookbook: wood and workshop1 beside the pose (make[stick], 4 ticks: max_timesteps
    12 is short for the generated worlds)."""
    ix = cb.index
    x, y = W // 2, H // 2
    rows = []
    if name == "limits":
        g = _ring(W, H, cb)
        g[x - 1, y], g[x + 1, y], g[x, y + 1], g[x, y - 1] = ix["glass"], ix["torch"], ix["rope"], ix["iron"]
        g[x, y - 2] = ix["workshop2"]
        g[1, 1], g[2, 1] = ix["workshop0"], ix["workshop1"]
        rows.append((g, x, y, 0, "make[lamp]"))
        g = _ring(W, H, cb)
        g[x - 1, y], g[x + 1, y], g[x, y + 1], g[x, y - 1] = ix["stick"], ix["coal"], ix["flax"], ix["workshop1"]
        g[1, 1], g[2, 1] = ix["workshop0"], ix["workshop2"]
        rows.append((g, x, y, 0, "make[torch]"))
        g = _ring(W, H, cb)
        g[x - 1, y], g[W - 2, H - 2], g[1, H - 2] = ix["crown"], ix["crown"], ix["crown"]
        g[1, 1], g[2, 1], g[3, 1] = ix["workshop0"], ix["workshop1"], ix["workshop2"]
        rows.append((g, x, y, 0, "get[crown]"))
        g = _ring(W, H, cb)
        g[x - 3, y - 1], g[W - 2, 1] = ix["glass"], ix["glass"]
        g[x + 1, y], g[x, y + 2] = ix["plank"], ix["gold"]
        g[1, 1], g[2, 1], g[3, 1] = ix["workshop0"], ix["workshop1"], ix["workshop2"]
        rows.append((g, x, y, 0, "get[glass]"))
        g = _ring(W, H, cb)
        g[x, y - 1], g[x + 2, y + 1] = ix["crown"], ix["crown"]
        g[1, 1], g[2, 1], g[3, 1] = ix["workshop0"], ix["workshop1"], ix["workshop2"]
        rows.append((g, x, y, 0, "make[crown]"))
    elif name == "k32compact":
        g = _ring(W, H, cb)
        g[x - 1, y], g[W - 2, H - 2], g[x + 2, y] = ix["ladder"], ix["ladder"], ix["fence"]
        g[1, 1], g[2, 1], g[3, 1] = ix["workshop0"], ix["workshop1"], ix["workshop2"]
        rows.append((g, x, y, 0, "get[ladder]"))
    g = _ring(W, H, cb)                                     # every cookbook: a stick within 4 ticks
    g[x - 1, y], g[x + 1, y], g[x, y + 2] = ix["wood"], ix["workshop1"], ix["iron"]
    g[1, 1], g[2, 1] = ix["workshop0"], ix["workshop2"]
    rows.append((g, x, y, 0, "make[stick]"))
    return rows


def cookbook_case(oracle_mod, name, world="w3", n=35, P=12, seed=11, max_timesteps=T_MAX, base=0):
    """Cookbook `name` on WORLDS[world]: P scenarios of the oracle's make_data generator over the
    cookbook's primitives and the hand_rows, and n env specs over them with tasks from the
    cookbook's whole get/make list; the first env on a hand-built row starts at its pose with its task.
    The fields of rect_cases.rect_case, and kw = CraftSim's recipes= / hints= (rect_cases.make_sim
    (case, device, **case.kw))."""
    W, H, window, prims = WORLDS[world]
    kw = yaml_paths(name)
    params, cb, tm, cfg = cookbook_tables(name, world, max_timesteps)
    assert cb.n_kinds == KINDS[name] and cfg.n_features == cb.n_kinds * (2 * window * window + 1) + 5
    ws = [cb.index["workshop%d" % i] for i in range(3)]
    pool, _, _ = oracle_mod.generate_scenarios(W, H, cb.index["boundary"], generator_primitives(cb), prims, ws,
                                               P, 123, rng="mt19937", dedup=True)
    hand = hand_rows(name, W, H, cb)
    pool = np.concatenate([pool, np.stack([h[0].reshape(-1) for h in hand])])
    tasks = [t.id for t in tm.dataset_tasks()]
    specs = [np.ascontiguousarray(a) for a in synthetic_specs(pool, W, H, n, base, seed=seed, task_ids=tasks)]
    for r, (_, x, y, d, task) in enumerate(hand):           # (the first env of each row: the later ones keep the list's tasks)
        on = (specs[0] == P + r) & (np.arange(n) < len(pool))
        specs[1][on], specs[2][on], specs[3][on], specs[4][on] = x, y, d, tm[task].id
    slots, no_slot = table_slots(cfg)
    return NS(tag=f"{name}-{world}", name=name, world=world, kw=kw, W=W, H=H, C=W * H, window=window, prims=prims,
              params=params, cb=cb, tm=tm, cfg=cfg, pool=pool, P=P, hand=hand, specs=specs, n=n, base=base,
              far_task=np.asarray([-1, -1], dtype=np.int32), max_timesteps=max_timesteps,
              crafted=sorted(cb.recipes.keys()), slots=slots, no_slot=no_slot,
              walk_tasks=sorted(t.id for t in tm.tasks if n_predicates(t) > 8))


def cookbook_actions(case):
    """rect_cases.mixed_actions, except that the envs on a hand-built row always follow the
    oracle's teacher, so that what the row was built for happens within its first episode."""
    def draw(o, envs, rng):
        acts = mixed_actions(o, envs, rng)
        for i in np.nonzero(envs["scenario"][:len(case.pool)] >= case.P)[0]:
            rc, a = o.teacher(envs[i:i + 1], int(envs["task"][i]))
            if rc == 0:
                acts[i] = a
        return acts
    return draw


def fp32_tail(n, tile, F):
    """Whether the last (partial) tile of n envs ends off a 16-byte boundary in fp32, so that
    stream_obs's scalar tail stores its last values."""
    return (n % tile) * F % 4 != 0


class CookbookCoverage:
    """What a run on a cookbook_case has exercised, from the oracle's envs, observations and
    labels (the `watch` of the rect_cases runners).  ticks / teacher: which families of condition
    check() asserts (a run without given teacher actions crafts nothing on purpose)."""

    def __init__(self, case, oracle_mod, ticks=True, teacher=False, crafts=True):
        self.c, self.o = case, oracle_mod.Oracle(case.cfg)
        self.ticks, self.teacher, self.crafts = ticks, teacher, crafts
        self.stop = self.timeout = self.restart = 0
        self.inv_top = self.window_top = self.task60 = 0
        self.fired = {}                                     # n_inputs -> times a recipe of that size fired
        self.slot14 = self.no_slot = self.walk = 0

    def tick(self, pre, acts, envs, done, autoreset, obs):
        c = self.c
        K, ww = c.cfg.n_kinds, c.window * c.window
        ended = done == 1
        live = pre["frozen"] == 0
        self.stop += int((ended & live & (acts == N.STOP)).sum())
        self.timeout += int((ended & live & (acts != N.STOP)).sum())
        if autoreset:
            self.restart += int((ended & (envs["timer"] == c.max_timesteps)).sum())
        self.inv_top += int((envs["inv"][:, K - 1] > 0).sum())
        self.window_top += int((obs[:, :ww * K].reshape(len(obs), ww, K)[:, :, K - 1] > 0).any(axis=1).sum())
        self.task60 += int((envs["task"] >= 60).sum())
        same_grid = (pre["grid"] == envs["grid"]).all(axis=1)
        for r in range(c.cfg.n_recipes):
            rc = c.cfg.recipe[r]
            made = ~ended & live & same_grid & (envs["inv"][:, rc.output] > pre["inv"][:, rc.output])
            for i in range(rc.n_inputs):                    # (this recipe, not another with the same output)
                made &= envs["inv"][:, rc.input_kind[i]] < pre["inv"][:, rc.input_kind[i]]
            self.fired[rc.n_inputs] = self.fired.get(rc.n_inputs, 0) + int(made.sum())

    def query(self, envs, labels):
        c = self.c
        for i in np.nonzero(np.asarray(labels) >= 0)[0]:
            task = c.tm.tasks[int(envs["task"][i])]
            self.walk += task.id in c.walk_tasks
            leaf = hint_leaf(self.o, envs[i:i + 1], task)
            if leaf is not None and leaf.goal_name == "go":
                k = c.cb.index[leaf.goal_arg]
                self.slot14 += c.slots.get(k) == 14
                self.no_slot += k in c.no_slot

    def check(self):
        c, what = self.c, {k: v for k, v in vars(self).items() if k not in ("c", "o")}
        if self.ticks:
            assert self.stop > 0 and self.timeout > 0 and self.restart > 0, what
            if c.name in ("limits", "k32compact"):
                assert self.inv_top > 0 and self.window_top > 0, what
            if c.name == "limits":
                assert self.task60 > 0, what
                if self.crafts:
                    assert self.fired.get(4, 0) > 0 and self.fired.get(3, 0) > 0, what
        if self.teacher and c.name == "limits":
            assert self.slot14 > 0 and self.no_slot > 0 and self.walk > 0, what
