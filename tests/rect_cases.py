"""Shared by tests/test_rect_worlds.py and tests/test_gpu_rect_worlds.py: worlds with
WIDTH != HEIGHT (tests/helpers.py RECT_SHAPES), their pools and specs, the lockstep of a simulator
against the oracle, and the conditions a run asserts it has exercised.  Every condition is computed
from the oracle's side (its envs, the actions given to both sides), never from the simulator under
test."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from psketch_amd import _native as N
from psketch_amd import synthetic_specs
from psketch_amd.cookbook import generator_primitives
from psketch_amd.sim import hash_actions
from tests.helpers import RECT_SHAPES, rect_tables

FULL_BAND = ("r6x16", "r10x16", "r12x16")      # (W-2)*H fills the teacher's bitset to its last bit
WIDE_WINDOW = ("r5x16", "r16x5")               # the window is larger than the world
FORMATS = ("f32", "bf16", "u8")


def edge_rows(W, H, cb):
    """Two hand-built pool rows whose only wood (row 0) / only iron (row 1) lies in the cell with
    the highest index of the teacher's band, (W-2, H-2): the last live bit of a full bitset."""
    ix = cb.index
    rows = []
    for far, near in (("wood", "iron"), ("iron", "wood")):
        g = np.zeros((W, H), dtype=np.uint8)
        g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = ix["boundary"]
        g[W - 2, H - 2] = ix[far]
        g[W - 2, 1] = ix[near]
        g[1, H - 2] = ix["grass"]
        g[1, 1], g[2, 1], g[1, H // 2] = ix["workshop0"], ix["workshop1"], ix["workshop2"]
        rows.append(g.reshape(-1))
    return np.stack(rows)


def rect_case(oracle_mod, tag, n=200, P=24, seed=11, max_timesteps=40, base=0):
    """The world of RECT_SHAPES[tag]: P scenarios of the oracle's make_data generator (numpy's
    RandomState stream, de-duplicated) and the two edge_rows, and n env specs over them; the envs
    on the edge rows have the task get[wood] / get[iron], whose target is the row's far cell."""
    W, H, window, prims = RECT_SHAPES[tag]
    params, cb, tm, cfg = rect_tables(tag, max_timesteps)
    ws = [cb.index["workshop%d" % i] for i in range(3)]
    pool, init, _ = oracle_mod.generate_scenarios(W, H, cb.index["boundary"], generator_primitives(cb), prims, ws,
                                                  P, 123, rng="mt19937", dedup=True)
    pool = np.concatenate([pool, edge_rows(W, H, cb)])
    specs = [np.ascontiguousarray(a) for a in
             synthetic_specs(pool, W, H, n, base, seed=seed, task_ids=[t.id for t in tm.dataset_tasks()])]
    far_task = np.asarray([tm["get[wood]"].id, tm["get[iron]"].id], dtype=np.int32)
    on_edge = specs[0] >= P
    specs[4][on_edge] = far_task[specs[0][on_edge] - P]
    return NS(tag=tag, W=W, H=H, C=W * H, window=window, prims=prims, params=params, cb=cb, tm=tm, cfg=cfg,
              pool=pool, P=P, specs=specs, n=n, base=base, far_task=far_task, max_timesteps=max_timesteps,
              crafted=sorted(cb.recipes.keys()))


def host(t):
    return t.cpu().numpy()


def make_sim(case, device, n=None, **kw):
    from psketch_amd import CraftSim
    sim = CraftSim(case.params, n_envs=case.n if n is None else n, device=device, pool_capacity=len(case.pool),
                   max_timesteps=case.max_timesteps, env_id_base=case.base, **kw)
    sim.load_pool(case.pool)
    return sim


def oracle_envs(oracle_mod, case):
    o = oracle_mod.Oracle(case.cfg, case.pool)
    return o, o.init_envs(*case.specs)


def mixed_actions(o, envs, rng, p_teacher=0.5, p=(.22, .22, .22, .22, .10, .02)):
    """Actions from the oracle's side: the DemonstrationTeacher's for about half the envs (so that
    items get crafted and episodes end on STOP), a seeded draw for the rest (blocked moves,
    timeouts)."""
    n = len(envs)
    acts = rng.choice(6, size=n, p=p).astype(np.int32)
    follow = rng.rand(n) < p_teacher
    for i in np.nonzero(follow)[0]:
        rc, a = o.teacher(envs[i:i + 1], int(envs["task"][i]))
        if rc == 0:
            acts[i] = a
    return acts


class LockstepCoverage:
    """What a lockstep run has exercised, from the oracle's envs before and after each tick."""

    def __init__(self, case):
        self.c = case
        self.stop = self.timeout = self.restart = self.cleared = self.crafted = 0
        self.col = self.row = 0
        self.blocked = dict(left=0, right=0, down=0, up=0)

    def tick(self, pre, acts, envs, done, autoreset):
        c = self.c
        ended = done == 1
        was_frozen = pre["frozen"] != 0
        self.stop += int((ended & ~was_frozen & (acts == N.STOP)).sum())
        self.timeout += int((ended & ~was_frozen & (acts != N.STOP)).sum())
        if autoreset:
            self.restart += int((ended & (envs["timer"] == c.max_timesteps)).sum())
        self.cleared += int((envs["grid"][:, :c.C] != c.pool[envs["scenario"]]).any(axis=1).sum())
        self.crafted += int((envs["inv"][:, c.crafted] > 0).any(axis=1).sum())
        self.col += int((envs["x"] == c.W - 2).sum())
        self.row += int((envs["y"] == c.H - 2).sum())
        stayed = ~ended & (pre["x"] == envs["x"]) & (pre["y"] == envs["y"])
        self.blocked["left"] += int((stayed & (acts == N.LEFT) & (pre["x"] == 1)).sum())
        self.blocked["right"] += int((stayed & (acts == N.RIGHT) & (pre["x"] == c.W - 2)).sum())
        self.blocked["down"] += int((stayed & (acts == N.DOWN) & (pre["y"] == 1)).sum())
        self.blocked["up"] += int((stayed & (acts == N.UP) & (pre["y"] == c.H - 2)).sum())

    def check(self):
        assert self.stop > 0 and self.timeout > 0 and self.restart > 0, vars(self)
        assert self.cleared > 0 and self.crafted > 0, vars(self)
        assert self.col > 0 and self.row > 0 and all(v > 0 for v in self.blocked.values()), vars(self)


class TeacherCoverage:
    """What the teacher queries of a run have exercised: states = the oracle's envs at a query,
    labels = the oracle's labels of those states (-1 for an env that was not queried)."""

    def __init__(self, case):
        self.c = case
        self.values = set()
        self.cleared = self.col = self.far = 0

    def query(self, envs, labels):
        c = self.c
        q = np.asarray(labels) != -1
        self.values |= set(np.asarray(labels)[q].tolist())
        self.cleared += int(((envs["grid"][:, :c.C] != c.pool[envs["scenario"]]).any(axis=1) & q).sum())
        self.col += int(((envs["x"] == c.W - 2) & q).sum())
        far_cell = (c.W - 2) * c.H + c.H - 2
        for r, kind in enumerate(("wood", "iron")):
            k = c.cb.index[kind]
            self.far += int((q & (envs["scenario"] == c.P + r) & (envs["task"] == c.far_task[r]) &
                             (envs["grid"][:, far_cell] == k) & (envs["inv"][:, k] == 0)).sum())

    def check(self):
        assert self.values >= set(range(6)), self.values
        assert self.cleared > 0, "no teacher query on a grid with a cleared cell"
        if self.c.tag in FULL_BAND:
            assert self.col > 0 and self.far > 0, vars(self)


def oracle_labels(o, envs):
    """oracle.teacher of every env's state and task: -1 for a frozen env, -2 where the reference
    raises."""
    out = np.empty(len(envs), dtype=np.int32)
    for i in range(len(envs)):
        if envs["frozen"][i]:
            out[i] = -1
        else:
            rc, a = o.teacher(envs[i:i + 1], int(envs["task"][i]))
            out[i] = -2 if rc else a
    return out


def check_teacher_latch(sim, labels):
    """CRAFT_ETEACHER is latched exactly when the oracle's teacher raised (-2) for a queried env."""
    try:
        sim.check()
    except N.CraftError as e:
        assert e.status == N.ETEACHER and (np.asarray(labels) == -2).any()
    else:
        assert not (np.asarray(labels) == -2).any()


def assert_state_equals_oracle(sim, envs, case):
    st = sim.get_state()
    np.testing.assert_array_equal(host(st["agent"]), np.stack([envs["x"], envs["y"], envs["dir"], envs["timer"]], 1))
    np.testing.assert_array_equal(host(st["inventory"]), envs["inv"][:, :case.cfg.n_kinds])
    np.testing.assert_array_equal(host(st["grid"]), envs["grid"][:, :case.C])


def run_lockstep(sim, case, oracle_mod, fmt="f32", T=45, teacher_at=(), autoreset=True, hashed_every=5,
                 actions=mixed_actions, watch=None):
    """craft_step on `sim` against the oracle every tick: observation (in format fmt), reward,
    done, success; at the ticks of teacher_at also standalone craft_teacher of every env against
    oracle.teacher; at the end agent / inventory / grid and stats.  actions: what draws the given
    actions from the oracle's side (mixed_actions); watch: a further coverage object, told every
    tick (tick(pre, acts, envs, done, autoreset, obs)) and teacher query (query(envs, labels)) of
    the oracle's and checked at the end."""
    n, dev = case.n, sim.device
    sim.set_obs_format(fmt)
    sim.reset(*case.specs)
    o, envs = oracle_envs(oracle_mod, case)
    obs = sim.empty_obs()
    rew = torch.empty(n, dtype=torch.float32, device=dev)
    done = torch.empty(n, dtype=torch.uint8, device=dev)
    succ = torch.empty(n, dtype=torch.int8, device=dev)
    rng = np.random.RandomState(case.W * 16 + case.H)
    stats = np.zeros(3, dtype=np.int64)
    cov, tcov = LockstepCoverage(case), TeacherCoverage(case)
    gids = np.arange(case.base, case.base + n)
    for t in range(T):
        pre = envs.copy()
        if hashed_every and t % hashed_every == hashed_every - 1:       # the in-kernel hashed draw
            given, acts = None, hash_actions(5, gids, t)
        else:
            given = acts = actions(o, envs, rng)
        sim.step(None if given is None else torch.as_tensor(given, device=dev), seed=5, tick=t,
                 autoreset=autoreset, obs=obs, reward=rew, done=done, success=succ)
        rc, oobs, orew, odone, osucc = o.batch_tick(envs, case.base, given, 5, t, autoreset, True, stats)
        assert rc == 0
        np.testing.assert_array_equal(host(done), odone, err_msg=f"done t={t}")
        np.testing.assert_array_equal(host(succ), osucc, err_msg=f"success t={t}")
        np.testing.assert_array_equal(host(rew), orew, err_msg=f"reward t={t}")
        np.testing.assert_array_equal(host(obs.float()), oobs, err_msg=f"obs t={t}")
        cov.tick(pre, acts, envs, odone, autoreset)
        if watch is not None:
            watch.tick(pre, acts, envs, odone, autoreset, oobs)
        if t in teacher_at:
            want = oracle_labels(o, envs)
            got, _ = sim.teacher()
            np.testing.assert_array_equal(host(got), want, err_msg=f"teacher t={t}")
            check_teacher_latch(sim, want)
            tcov.query(envs, want)
            if watch is not None:
                watch.query(envs, want)
            assert_state_equals_oracle(sim, envs, case)
    assert_state_equals_oracle(sim, envs, case)
    np.testing.assert_array_equal(host(sim.stats()), stats)
    sim.check()
    cov.check()
    if teacher_at:
        tcov.check()
    if watch is not None:
        watch.check()
    return cov, tcov


def run_rollout(sim, case, oracle_mod, fmt="f32", launches=4, K=12, R=None, hashed=(1,), actions=mixed_actions,
                watch=None):
    """craft_rollout on `sim`, `launches` launches of K ticks, against the oracle's per-tick
    results: every slot of the observation / reward / done / success rings after each launch (ring
    R ticks, default K: a shorter ring holds the launch's last R ticks), the state after each
    launch and stats.  The launches of `hashed` use the in-kernel hashed draw, the others a table
    of `actions` (mixed_actions); watch as in run_lockstep."""
    n, dev = case.n, sim.device
    R = K if R is None else R
    sim.set_obs_format(fmt)
    sim.reset(*case.specs)
    o, envs = oracle_envs(oracle_mod, case)
    obs = torch.zeros((R, n, sim.n_features), dtype=sim.obs_dtype, device=dev)
    rew = torch.zeros((R, n), dtype=torch.float32, device=dev)
    done = torch.zeros((R, n), dtype=torch.uint8, device=dev)
    succ = torch.zeros((R, n), dtype=torch.int8, device=dev)
    rng = np.random.RandomState(case.W * 16 + case.H + 1)
    stats = np.zeros(3, dtype=np.int64)
    cov = LockstepCoverage(case)
    gids = np.arange(case.base, case.base + n)
    for l in range(launches):
        table, want = [], {}
        for t in range(l * K, (l + 1) * K):
            pre = envs.copy()
            if l in hashed:
                given, acts = None, hash_actions(5, gids, t)
            else:
                given = acts = actions(o, envs, rng)
                table.append(given)
            rc, *res = o.batch_tick(envs, case.base, given, 5, t, True, True, stats)
            assert rc == 0
            want[t % R] = (t, res)
            cov.tick(pre, acts, envs, res[2], True)
            if watch is not None:
                watch.tick(pre, acts, envs, res[2], True, res[0])
        sim.rollout(K, seed=5, tick0=l * K, actions=torch.as_tensor(np.stack(table), device=dev) if table else None,
                    autoreset=True, obs=obs, reward=rew, done=done, success=succ)
        for slot, (t, (oobs, orew, odone, osucc)) in want.items():
            np.testing.assert_array_equal(host(obs[slot].float()), oobs, err_msg=f"obs t={t}")
            np.testing.assert_array_equal(host(rew[slot]), orew, err_msg=f"reward t={t}")
            np.testing.assert_array_equal(host(done[slot]), odone, err_msg=f"done t={t}")
            np.testing.assert_array_equal(host(succ[slot]), osucc, err_msg=f"success t={t}")
        assert_state_equals_oracle(sim, envs, case)
    np.testing.assert_array_equal(host(sim.stats()), stats)
    sim.check()
    cov.check()
    if watch is not None:
        watch.check()
    return cov


def run_step_teach(sim, case, oracle_mod, T=30, watch=None):
    """craft_step_teach on `sim` (craft_step with labels): the label of every env every tick
    against oracle.teacher, the observation against the oracle; given actions with USE at about
    35 %, so cells are cleared and queries leave the teacher table; watch as in run_lockstep."""
    n, dev = case.n, sim.device
    sim.reset(*case.specs)
    o, envs = oracle_envs(oracle_mod, case)
    obs = sim.empty_obs()
    lab = torch.empty(n, dtype=torch.int32, device=dev)
    rng = np.random.RandomState(case.W * 16 + case.H + 2)
    tcov = TeacherCoverage(case)
    for t in range(T):
        acts = rng.choice(6, size=n, p=[.15, .15, .15, .15, .38, .02]).astype(np.int32)
        pre = envs.copy()
        sim.step(torch.as_tensor(acts, device=dev), seed=3, tick=t, autoreset=True, obs=obs, labels=lab)
        rc, oobs, _, odone, _ = o.batch_tick(envs, case.base, acts, 3, t, True, True, None)
        assert rc == 0
        want = oracle_labels(o, envs)
        if watch is not None:
            watch.tick(pre, acts, envs, odone, True, oobs)
            watch.query(envs, want)
        np.testing.assert_array_equal(host(lab), want, err_msg=f"labels t={t}")
        np.testing.assert_array_equal(host(obs.float()), oobs, err_msg=f"obs t={t}")
        check_teacher_latch(sim, want)
        tcov.query(envs, want)
    assert_state_equals_oracle(sim, envs, case)
    tcov.check()
    if watch is not None:
        watch.check()
    return tcov
