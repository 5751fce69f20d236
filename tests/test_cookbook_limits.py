"""Cookbooks up to the ABI's limits on the CPU (tests/cookbook_cases.py: 32 kinds, 16 recipes of up
to 4 ingredients, 64 tasks of up to 4 subtasks; 22 and 12 kinds, whose observation rows are odd):
the oracle and the CPU variant of the C ABI against the reference's own results on those cookbooks
(tests/golden/cookbook_limits.npz, written by `python tests/golden/make_golden.py limits`), the CPU
variant against the oracle with the runners of tests/rect_cases.py, and what compile_config and
craft_sim_create refuse one past each limit.  tests/test_gpu_cookbook_limits.py runs the HIP kernels
on the same cases."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from psketch_amd import CraftSim, sample_scenarios
from psketch_amd import _native as N
from psketch_amd.cookbook import Cookbook, TaskManager, compile_config, generator_primitives, world_params
from tests.cookbook_cases import (COOKBOOKS, FIXTURE_WORLD, KINDS, T_MAX, WORLDS, CookbookCoverage, cookbook_actions,
                                  cookbook_case, cookbook_tables, cookbook_world, fp32_tail, n_predicates,
                                  table_slots, yaml_paths)
from tests.rect_cases import (check_teacher_latch, host, make_sim, oracle_labels, run_lockstep, run_rollout,
                              run_step_teach)
from tests.test_gpu_parity import set_states
from tests.test_rect_worlds import check_distances_vs_oracle, check_kats, check_teach_rollout, teach_reference


@pytest.fixture(scope="module")
def fx(golden):
    return golden("cookbook_limits.npz")


# ---- the cookbooks are what their names say -----------------------------------------------------
def test_cookbooks_reach_the_limits_they_are_named_for():
    for name in COOKBOOKS:
        for world, (W, H, window, _) in WORLDS.items():
            _, cb, tm, cfg = cookbook_tables(name, world)
            assert cb.n_kinds == KINDS[name] and cfg.n_features == KINDS[name] * (2 * window * window + 1) + 5
        for k in ("boundary", "workshop0", "workshop1", "workshop2", "water", "stone", "bridge", "axe"):
            assert cb.index[k], (name, k)
        assert not any(cfg.task[t].arg_kind == cb.index["boundary"] for t in range(cfg.n_tasks))
    F = {n: [cookbook_tables(n, w)[3].n_features for w in WORLDS] for n in COOKBOOKS}
    assert F["limits"] == [613, 1637, 3173] and F["even"] == [423, 1127, 2183] and F["tiny"][0] == 233
    for name in ("limits", "even", "tiny"):                  # the fp32 scalar tail of a 3- and a 6-env tail tile
        for n in (35, 70):
            assert all(fp32_tail(n, tile, f) for tile in (16, 32, 64) for f in F[name]), name

    _, cb, tm, cfg = cookbook_tables("limits")
    rec = [cfg.recipe[r] for r in range(cfg.n_recipes)]
    per_ws = {}
    for r in rec:
        per_ws[r.workshop] = per_ws.get(r.workshop, 0) + 1
    assert (cfg.n_kinds, cfg.n_recipes, cfg.n_tasks) == (N.MAX_KINDS, N.MAX_RECIPES, N.MAX_TASKS)
    assert max(per_ws.values()) >= 4                         # no compact per-workshop table
    assert sorted({r.n_inputs for r in rec}) == [1, 2, 3, 4] and any(r.yield_ > 1 for r in rec)
    made = {}
    chained = False
    for r in rec:                                            # an ingredient an earlier recipe of the workshop makes
        chained |= any(made.get(r.input_kind[i]) == r.workshop for i in range(r.n_inputs))
        made[r.output] = r.workshop
    assert chained
    top = cb.index["crown"]
    assert top == 31 and top not in cb.environment and rec[-1].output == top
    assert {(t.goal_name) for t in tm.tasks if t.goal_arg == "crown"} >= {"go", "get", "make"}
    slots, no_slot = table_slots(cfg)
    assert len(slots) == 15 and len(no_slot) >= 2 and slots[top] == 14
    assert max(len(t.subtasks or []) for t in tm.tasks) == N.MAX_SUBTASKS
    assert any(t.id >= 60 and t.subtasks and t.goal_name in ("get", "make") for t in tm.tasks)
    assert n_predicates(tm["make[lamp]"]) > 8

    _, cb, tm, cfg = cookbook_tables("k32compact")
    rec = [cfg.recipe[r] for r in range(cfg.n_recipes)]
    assert cfg.n_kinds == 32 and cfg.n_recipes == 9 and max(r.n_inputs for r in rec) <= 2
    assert all(sum(1 for r in rec if r.workshop == w) <= 3 for w in {r.workshop for r in rec})
    assert cb.index["ladder"] == 31 and list(cfg.kind_class).count(N.KIND_INERT) >= 8


# ---- the oracle against the reference -----------------------------------------------------------
@pytest.mark.parametrize("name", COOKBOOKS)
def test_oracle_random_step_kats(fx, oracle_mod, name):
    W, H, _, _ = WORLDS[FIXTURE_WORLD[name]]
    _, cb, tm, cfg = cookbook_tables(name, FIXTURE_WORLD[name])
    o = oracle_mod.Oracle(cfg)
    p = f"{name}_kat_"
    K = cfg.n_kinds
    assert fx[p + "pre_grid"].shape[1] == W * H and fx[p + "features"].shape[1] == cfg.n_features
    assert fx[p + "satisfies"].shape[1] == len(tm) and fx[p + "pre_inv"].shape[1] == K
    if K == 32:                                              # kind 31 on the grids, held, grabbed
        assert (fx[p + "pre_grid"] == 31).any() and (fx[p + "pre_inv"][:, 31] > 0).any()
        assert (fx[p + "post_inv"][:, 31] > fx[p + "pre_inv"][:, 31]).any()
    for i in range(len(fx[p + "action"])):
        x, y, d = (int(v) for v in fx[p + "pre_agent"][i])
        env = o.env(fx[p + "pre_grid"][i], x, y, d, fx[p + "pre_inv"][i])
        np.testing.assert_array_equal(o.features(env), fx[p + "features"][i], err_msg=str(i))
        assert [o.satisfies(env, t) for t in range(len(tm))] == fx[p + "satisfies"][i].tolist(), i
        assert o.step(env, int(fx[p + "action"][i])) == 0
        assert [int(env["x"][0]), int(env["y"][0]), int(env["dir"][0])] == fx[p + "post_agent"][i].tolist(), i
        assert env["inv"][0, :K].tolist() == fx[p + "post_inv"][i].tolist(), i
        assert env["grid"][0, :W * H].tolist() == fx[p + "post_grid"][i].tolist(), i


@pytest.mark.parametrize("name", COOKBOOKS)
def test_oracle_teacher(fx, oracle_mod, name):
    _, cb, tm, cfg = cookbook_tables(name, FIXTURE_WORLD[name])
    o = oracle_mod.Oracle(cfg)
    p = f"{name}_teacher_"
    assert fx[p + "action"].shape[1] == len(tm)
    if cfg.n_kinds == 32:
        assert (fx[p + "grid"] == 31).any() and (fx[p + "inv"][:, 31] > 0).any()
    for i in range(len(fx[p + "grid"])):
        x, y, d = fx[p + "agent"][i]
        env = o.env(fx[p + "grid"][i], x, y, d, fx[p + "inv"][i])
        for t in range(len(tm)):
            rc, a = o.teacher(env, t)
            ref = int(fx[p + "action"][i, t])
            if ref == -2:
                assert rc == N.ETEACHER, (i, t)
            else:
                assert rc == 0 and a == ref, (i, t, a, ref)
            ref_len = int(fx[p + "path_len"][i, t])
            if ref_len != -3:
                rc, _, ln = o.closest_resource(env, cfg.task[t].arg_kind)
                if ref_len == -2:
                    assert rc == N.ETEACHER
                else:
                    assert rc == 0 and ln == ref_len, (i, t, ln, ref_len)


@pytest.mark.parametrize("name", COOKBOOKS)
def test_oracle_rollout(fx, oracle_mod, name):
    W, H, _, _ = WORLDS[FIXTURE_WORLD[name]]
    _, _, tm, cfg = cookbook_tables(name, FIXTURE_WORLD[name])
    p = f"{name}_rollout_"
    o = oracle_mod.Oracle(cfg, fx[p + "pool"])
    sp = fx[p + "spec"]
    envs = o.init_envs(sp[:, 0], sp[:, 1], sp[:, 2], sp[:, 3], sp[:, 4])
    seed = int(fx[p + "seed"][0])
    T = fx[p + "done"].shape[0]
    assert fx[p + "obs_ticks"].tolist() == list(range(T)) and T > 2 * cfg.max_timesteps      # timeouts occur
    for t in range(T):
        rc, obs, reward, done, success = o.batch_tick(envs, 0, None, seed, t, True)
        assert rc == 0
        np.testing.assert_array_equal(obs, fx[p + "obs"][t], err_msg=f"obs t={t}")
        np.testing.assert_array_equal(reward, fx[p + "reward"][t])
        np.testing.assert_array_equal(done, fx[p + "done"][t])
        np.testing.assert_array_equal(success, fx[p + "success"][t])
        np.testing.assert_array_equal(np.stack([envs["x"], envs["y"], envs["dir"], envs["timer"]], 1), fx[p + "agent"][t])
        np.testing.assert_array_equal(envs["inv"][:, :cfg.n_kinds], fx[p + "inv"][t])
        np.testing.assert_array_equal(envs["grid"][:, :W * H], fx[p + "grid"][t])


@pytest.mark.parametrize("name", COOKBOOKS)
def test_scenario_generators_reproduce_reference_stream(fx, oracle_mod, name):
    """make_data.sample_scenario over each cookbook's primitives (the set's iteration order)."""
    W, H, _, prims = WORLDS[FIXTURE_WORLD[name]]
    params, cb, _, _ = cookbook_tables(name, FIXTURE_WORLD[name])
    p = f"{name}_scen_"
    count = len(fx[p + "grids"])
    ws = [cb.index["workshop%d" % i] for i in range(3)]
    native = sample_scenarios(params, cb, 123, count)
    c_oracle = oracle_mod.generate_scenarios(W, H, cb.index["boundary"], generator_primitives(cb), prims, ws, count,
                                             123, rng="mt19937", dedup=True)
    for grids, init, mt in (native, c_oracle):
        np.testing.assert_array_equal(grids, fx[p + "grids"])
        np.testing.assert_array_equal(init, fx[p + "init"])
        assert np.array_equal(mt[:624], fx[p + "mt_key"]) and mt[624] == fx[p + "mt_pos"][0]


# ---- the ABI against the reference (shared with the GPU file) -----------------------------------
def check_fixture_kats(fx, name, device):
    check_kats(fx, name, device, world=cookbook_world(FIXTURE_WORLD[name]), **yaml_paths(name))


def check_fixture_teacher(fx, name, device):
    """craft_teacher with path_len_out on the fixture's states, every task of the cookbook."""
    p = f"{name}_teacher_"
    n = len(fx[p + "grid"])
    sim = CraftSim(cookbook_world(FIXTURE_WORLD[name]), n_envs=n, device=device, pool_capacity=n, **yaml_paths(name))
    sim.load_pool(fx[p + "grid"])
    set_states(sim, np.arange(n), fx[p + "agent"], fx[p + "inv"])
    dev = sim.device
    plen = torch.empty(n, dtype=torch.int32, device=dev)
    for table in (1, 2):
        sim.tune_teach(0, 0, table)
        for t in range(fx[p + "action"].shape[1]):
            a, _ = sim.teacher(tasks=torch.full((n,), t, dtype=torch.int32, device=dev), path_len_out=plen, n=n)
            np.testing.assert_array_equal(host(a), fx[p + "action"][:, t], err_msg=f"task {t}")
            ref = fx[p + "path_len"][:, t]
            if (ref != -3).all():
                np.testing.assert_array_equal(host(plen), ref, err_msg=f"task {t}")
            # (the path length of a satisfied task's target can raise where its action does not)
            check_teacher_latch(sim, np.concatenate([fx[p + "action"][:, t], ref]))


def check_fixture_rollout(fx, name, device):
    p = f"{name}_rollout_"
    sp = fx[p + "spec"]
    E = len(sp)
    sim = CraftSim(cookbook_world(FIXTURE_WORLD[name]), n_envs=E, device=device, pool_capacity=len(fx[p + "pool"]),
                   max_timesteps=T_MAX, **yaml_paths(name))
    sim.load_pool(fx[p + "pool"])
    sim.reset(sp[:, 0], sp[:, 1], sp[:, 2], sp[:, 3], sp[:, 4])
    dev = sim.device
    obs = sim.empty_obs()
    rew = torch.empty(E, dtype=torch.float32, device=dev)
    done = torch.empty(E, dtype=torch.uint8, device=dev)
    succ = torch.empty(E, dtype=torch.int8, device=dev)
    seed = int(fx[p + "seed"][0])
    for t in range(fx[p + "done"].shape[0]):
        sim.step(seed=seed, tick=t, obs=obs, reward=rew, done=done, success=succ)
        st = sim.get_state()
        np.testing.assert_array_equal(host(done), fx[p + "done"][t])
        np.testing.assert_array_equal(host(succ), fx[p + "success"][t])
        np.testing.assert_array_equal(host(rew), fx[p + "reward"][t].astype(np.float32))
        np.testing.assert_array_equal(host(st["agent"]), fx[p + "agent"][t])
        np.testing.assert_array_equal(host(st["inventory"]), fx[p + "inv"][t][:, :sim.n_kinds])
        np.testing.assert_array_equal(host(st["grid"]), fx[p + "grid"][t])
        np.testing.assert_array_equal(host(obs), fx[p + "obs"][t].astype(np.float32), err_msg=f"obs t={t}")
    sim.check()


@pytest.mark.parametrize("name", COOKBOOKS)
def test_fixture_cpu(fx, name):
    check_fixture_kats(fx, name, "cpu")
    check_fixture_teacher(fx, name, "cpu")
    check_fixture_rollout(fx, name, "cpu")


# ---- the ABI against the oracle (shared with the GPU file) --------------------------------------
# cookbook, world, format: all four at window 3, limits and even at every window and in every format
LOCKSTEP_ROWS = [("limits", "w3", "f32"), ("k32compact", "w3", "f32"), ("even", "w3", "f32"), ("tiny", "w3", "f32"),
                 ("limits", "w5", "f32"), ("limits", "w7", "f32"), ("even", "w5", "f32"), ("even", "w7", "f32"),
                 ("limits", "w3", "bf16"), ("limits", "w7", "u8"), ("even", "w3", "u8"), ("even", "w5", "bf16"),
                 ("limits", "w5", "u8"), ("even", "w7", "bf16")]


def lockstep(oracle_mod, device, name, world, fmt, n=35, T=36, tile=0):
    """craft_step against the oracle with the teacher's actions on the hand-built rows (ticks 12
    and 25 use the hashed draw: the rows' first episode, ticks 0..11, is undisturbed) and
    craft_teacher of every env at three ticks."""
    case = cookbook_case(oracle_mod, name, world, n=n)
    sim = make_sim(case, device, **case.kw)
    if tile:
        sim.tune(tile_envs=tile, obs_store=2)
    run_lockstep(sim, case, oracle_mod, fmt=fmt, T=T, teacher_at=(0, 7, T - 1), hashed_every=13,
                 actions=cookbook_actions(case), watch=CookbookCoverage(case, oracle_mod, teacher=True))
    return sim


@pytest.mark.parametrize("name,world,fmt", LOCKSTEP_ROWS)
def test_lockstep_vs_oracle_cpu(oracle_mod, name, world, fmt):
    lockstep(oracle_mod, "cpu", name, world, fmt, n=70 if LOCKSTEP_ROWS.index((name, world, fmt)) % 2 else 35)


# Every slot of an observation ring must start on a 16-byte boundary, so with an odd row length the
# K-tick entry points take a multiple of 4 (f32), 8 (bf16) or 16 (u8) envs: a 32-env tile and a
# partial one, and two 32-env tiles (one 64-env tile) and a partial one.  A ring of one slot has no
# such rule: those rows keep 35 envs (`envs`), and their fp32 tail tile ends off a 16-byte boundary,
# so stream_obs's scalar tail runs in the K-tick kernels too.
RING_N = {"f32": (36, 68), "bf16": (40, 72), "u8": (48, 80)}


def rollout(oracle_mod, device, name, world, fmt, n=0, tile=0, threads=0, chunk=0, R=None, shape=None, envs=None):
    assert envs is None or R == 1
    # (spec seed 12 for the 35-env rows: with 11 no env of limits is blocked at the right border)
    case = cookbook_case(oracle_mod, name, world, n=envs or RING_N[fmt][n], seed=12 if envs else 11)
    sim = make_sim(case, device, **case.kw)
    if tile:
        sim.tune(tile_envs=tile, obs_store=2)
    sim.tune_rollout(chunk, threads)
    if shape is not None:
        assert sim.rollout_shape() == shape, sim.rollout_shape()
    run_rollout(sim, case, oracle_mod, fmt=fmt, launches=3, K=12, R=R, actions=cookbook_actions(case),
                watch=CookbookCoverage(case, oracle_mod))
    return sim


@pytest.mark.parametrize("name,world,fmt,R", [("limits", "w3", "f32", None), ("even", "w3", "u8", 5),
                                               ("limits", "w7", "bf16", None), ("even", "w5", "f32", None),
                                               ("limits", "w3", "f32", 1), ("even", "w3", "f32", 1)])
def test_rollout_vs_oracle_cpu(oracle_mod, name, world, fmt, R):
    rollout(oracle_mod, "cpu", name, world, fmt, R=R, envs=35 if R == 1 else None)


def step_teach(oracle_mod, device, name, world, n=70, kernel=0, lanes=0, table=0, shape=None):
    case = cookbook_case(oracle_mod, name, world, n=n)
    sim = make_sim(case, device, **case.kw)
    sim.tune_teach(kernel, lanes, table)
    if shape is not None:
        assert sim.step_shape(teach=True)[:2] == shape, sim.step_shape(teach=True)
    run_step_teach(sim, case, oracle_mod, T=24, watch=CookbookCoverage(case, oracle_mod, teacher=True, crafts=False))
    return sim


@pytest.mark.parametrize("name,world", [("limits", "w3"), ("limits", "w7"), ("even", "w5"), ("tiny", "w3"),
                                        ("k32compact", "w3")])
def test_step_teach_vs_oracle_cpu(oracle_mod, name, world):
    step_teach(oracle_mod, "cpu", name, world)


@functools.lru_cache(maxsize=None)
def case_maker(name, world):
    """rect_case's signature over cookbook_case, one object per (name, world): test_rect_worlds.
    teach_reference caches its references by it."""
    def make(oracle_mod, tag, n, seed, base):
        return cookbook_case(oracle_mod, name, world, n=n, seed=seed)     # (base 0: the tasks >= 60 stay off the hand-built rows)
    return make


@functools.lru_cache(maxsize=None)
def watch_maker(oracle_mod):
    return lambda case: CookbookCoverage(case, oracle_mod, teacher=True, crafts=False)


def rollout_teach(oracle_mod, device, name, world, mode, table=0, n=36):
    """Launches of craft_rollout_teach chaining label_in against rollout_oracle.teach_rollout
    (computed once per row): labels, action_record, done, success, observations, states.  Two
    launches of 16 ticks; in label mode, where nothing restarts and every env has stopped by tick
    12, three of 5."""
    launches, K = (3, 5) if mode == "label" else (2, 16)
    case, o, a, refs = teach_reference(oracle_mod, f"{name}-{world}", mode, n=n, launches=launches, K=K, want_obs=True,
                                       make_case=case_maker(name, world),
                                       make_watch=watch_maker(oracle_mod) if mode != "label" else None)
    sim = make_sim(case, device, **case.kw)
    sim.tune_teach(0, 0, table)
    check_teach_rollout(sim, case, a, refs, K=K)
    return sim


@pytest.mark.parametrize("mode", ["policy", "label", "bc"])
@pytest.mark.parametrize("name,world", [("limits", "w3"), ("limits", "w7"), ("even", "w3")])
def test_rollout_teach_cpu_vs_oracle(oracle_mod, name, world, mode):
    rollout_teach(oracle_mod, "cpu", name, world, mode)


def check_pool_generate(oracle_mod, name, world, device, count=24):
    """craft_pool_generate over the cookbook's primitives against the oracle's splitmix stream."""
    W, H, _, prims = WORLDS[world]
    sim = CraftSim(cookbook_world(world), n_envs=count, device=device, pool_capacity=count + 3, **yaml_paths(name))
    init = sim.generate_pool(count, seed=77, first=3, scenario_id0=500, init_pos=True)
    cb = sim.cookbook
    ws = [cb.index["workshop%d" % i] for i in range(3)]
    grids, oinit, _ = oracle_mod.generate_scenarios(W, H, cb.index["boundary"], generator_primitives(cb), prims, ws,
                                                    count, 77, rng="splitmix", scenario_id0=500)
    np.testing.assert_array_equal(host(init), oinit)
    z = np.zeros(count, np.int32)
    sim.reset(np.arange(3, 3 + count, dtype=np.int32), oinit[:, 0], oinit[:, 1], z, z)
    np.testing.assert_array_equal(host(sim.get_state()["grid"]), grids)
    assert all((grids == k).any() for k in generator_primitives(cb))
    sim.check()


def check_distances(oracle_mod, name, world, device):
    case = cookbook_case(oracle_mod, name, world)
    return check_distances_vs_oracle(oracle_mod, f"{name}-{world}", device, make_case=case_maker(name, world), n=68,
                                     **case.kw)


def test_pool_generate_and_distances_cpu(oracle_mod):
    check_pool_generate(oracle_mod, "limits", "w3", "cpu")
    check_distances(oracle_mod, "limits", "w3", "cpu")


# ---- kind 31 at the count limit -----------------------------------------------------------------
def check_top_kind_saturates(oracle_mod, device):
    """inv[31] = 255: grabbing a kind-31 cell (slot 1) and crafting kind 31 (slot 2) leave the
    count at 255, clear the cell / consume the ingredients as below 255, and latch CRAFT_ERANGE
    with the slot; slot 0, at 254, reaches 255 without a latch."""
    case = cookbook_case(oracle_mod, "limits", "w3", n=3)
    ix = case.cb.index
    W, H = case.W, case.H
    g = np.zeros((W, H), dtype=np.uint8)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = ix["boundary"]
    g[4, 5], g[6, 5] = ix["crown"], ix["workshop1"]
    sim = CraftSim(case.params, n_envs=3, device=device, pool_capacity=1, **case.kw)
    sim.load_pool(g.reshape(1, -1))
    inv = np.zeros((3, 32), dtype=np.int32)
    inv[:, 31] = (254, 255, 255)
    inv[2, ix["linen"]] = inv[2, ix["glass"]] = 2
    set_states(sim, [0, 0, 0], [[5, 5, N.LEFT], [5, 5, N.LEFT], [5, 5, N.RIGHT]], inv)
    use = torch.full((3,), N.USE, dtype=torch.int32, device=sim.device)
    for slot in (0, 1, 2):                                   # one slot a launch: each latch names its slot
        acts = torch.where(torch.arange(3, device=sim.device) == slot, use, torch.full_like(use, N.STOP))
        sim.transition(acts)
        w = host(sim.error_word()).tolist()
        if slot == 0:
            assert w[0] == 0
            sim.check()
        else:
            assert w[0] == N.ERANGE and w[2] == slot, w
            with pytest.raises(N.CraftError) as e:
                sim.check()
            assert e.value.status == N.ERANGE
    st = sim.get_state()
    got = host(st["inventory"])
    assert got[:, 31].tolist() == [255, 255, 255]
    assert got[2, ix["linen"]] == 1 and got[2, ix["glass"]] == 1
    grid = host(st["grid"]).reshape(3, W, H)
    assert grid[0, 4, 5] == 0 and grid[1, 4, 5] == 0 and grid[2, 4, 5] == ix["crown"]
    obs = sim.empty_obs()
    sim.observe(obs=obs)
    F = sim.n_features
    assert host(obs)[:, F - 5 - 32 + 31].tolist() == [255, 255, 255]     # byte 31 of the inventory row


def test_top_kind_saturates_cpu(oracle_mod):
    check_top_kind_saturates(oracle_mod, "cpu")


# ---- every ingredient of a long recipe counts ----------------------------------------------------
def check_recipes_need_every_ingredient(oracle_mod, device):
    """lamp (4 ingredients, workshop2), torch (3, workshop1) and kiln (2 bricks and an iron,
    workshop0): holding all ingredients makes the item; with any one ingredient missing, or one
    brick short, USE at the workshop changes nothing.  The expected inventories are the oracle's."""
    case = cookbook_case(oracle_mod, "limits", "w3", n=4)
    ix, cfg = case.cb.index, case.cfg
    W, H = case.W, case.H
    g = np.zeros((W, H), dtype=np.uint8)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = ix["boundary"]
    g[4, 5], g[6, 5], g[5, 6] = ix["workshop0"], ix["workshop1"], ix["workshop2"]
    face = {"workshop0": N.LEFT, "workshop1": N.RIGHT, "workshop2": N.UP}
    rows = []                                                # (dir, inventory, the item made or None)
    for item, ws in (("lamp", "workshop2"), ("torch", "workshop1"), ("kiln", "workshop0")):
        need = {k: v for k, v in case.cb.recipes[ix[item]].items() if isinstance(k, int)}
        full = np.zeros(32, dtype=np.int32)
        for k, v in need.items():
            full[k] = v
        rows.append((face[ws], full, ix[item]))
        for k in need:                                       # one short of each ingredient in turn
            inv = full.copy()
            inv[k] -= 1
            rows.append((face[ws], inv, None))
    n = len(rows)
    sim = CraftSim(case.params, n_envs=n, device=device, pool_capacity=1, **case.kw)
    sim.load_pool(g.reshape(1, -1))
    inv = np.stack([r[1] for r in rows])
    set_states(sim, [0] * n, [[5, 5, r[0]] for r in rows], inv)
    sim.transition(torch.full((n,), N.USE, dtype=torch.int32, device=sim.device))
    sim.check()
    got = host(sim.get_state()["inventory"])
    o = oracle_mod.Oracle(cfg)
    for i, (d, iv, made) in enumerate(rows):
        env = o.env(g, 5, 5, d, iv)
        assert o.step(env, N.USE) == 0
        want = env["inv"][0, :32]
        assert (want[made] == 1 and want.sum() == 1) if made else (want == iv).all(), i
        np.testing.assert_array_equal(got[i], want, err_msg=f"row {i}")


def test_recipes_need_every_ingredient_cpu(oracle_mod):
    check_recipes_need_every_ingredient(oracle_mod, "cpu")


# ---- a tile that cannot be carved ---------------------------------------------------------------
def check_tile_that_does_not_fit(oracle_mod, device):
    """include/craft.h craft_sim_tune: 64-env tiles of 32 kinds at 7x7 windows (203 KB of staged
    observation rows) are refused with CRAFT_EINVAL, the handle keeps its tile, and ticks with and
    without the teacher still equal the oracle; at 5x5 windows (125 KB) the tile is accepted."""
    case = cookbook_case(oracle_mod, "limits", "w7", n=70)
    sim = make_sim(case, device, **case.kw)
    before = sim.tile_shape()
    with pytest.raises(N.CraftError) as e:
        sim.tune(tile_envs=64, obs_store=2)
    assert e.value.status == N.EINVAL and "does not fit" in str(e.value)
    assert sim.tile_shape() == before == (32, 2)
    sim.tune(tile_envs=16, obs_store=2)                      # (the teacher's tick picks its own tile then)
    assert sim.tile_shape() == (16, 2) and sim.step_shape(teach=True)[1] in (16, 32)
    run_step_teach(sim, case, oracle_mod, T=13)
    run_lockstep(sim, case, oracle_mod, T=26, teacher_at=(3,), hashed_every=13, actions=cookbook_actions(case))
    case5 = cookbook_case(oracle_mod, "limits", "w5", n=70)
    sim5 = make_sim(case5, device, **case5.kw)
    sim5.tune(tile_envs=64, obs_store=2)
    assert sim5.tile_shape() == (64, 2)
    run_lockstep(sim5, case5, oracle_mod, T=26, hashed_every=13, actions=cookbook_actions(case5))
    small = CraftSim(case.params, n_envs=4, device=device, pool_capacity=1)      # 21 kinds: 64 envs fit (153 KB)
    small.tune(tile_envs=64, obs_store=2)


def test_tile_that_does_not_fit_cpu(oracle_mod):
    check_tile_that_does_not_fit(oracle_mod, "cpu")


# ---- one past each limit ------------------------------------------------------------------------
def _over(what):
    """(recipes, hints) dicts one past a limit of the ABI."""
    import copy

    import yaml
    paths = yaml_paths("limits")
    recipes, hints = (yaml.safe_load(open(paths[k])) for k in ("recipes", "hints"))
    recipes, hints = copy.deepcopy(recipes), dict(hints)
    if what == "kinds":
        recipes["primitives"].append("salt")
    elif what == "recipes":
        recipes["recipes"]["pole"] = {"stick": 2, "_at": "workshop1"}       # (and a 33rd kind)
        recipes["primitives"].remove("gem")
        hints = {k: v for k, v in hints.items() if "gem" not in k}
    elif what == "ingredients":
        recipes["recipes"]["lamp"]["coal"] = 1
    elif what == "tasks":
        hints["get[linen]"] = ["make[linen]"]
    elif what == "subtasks":
        hints["make[torch]"] = ["get[stick]", "get[coal]", "get[flax]", "go[workshop1]", "use[none]"]
    return recipes, hints


@pytest.mark.parametrize("what", ["kinds", "recipes", "ingredients", "tasks", "subtasks"])
def test_compile_config_refuses_one_past_each_limit(what):
    recipes, hints = _over(what)
    cb, tm = Cookbook(recipes), TaskManager(hints)
    assert {"kinds": cb.n_kinds == 33, "recipes": len(cb.recipes) == 17 and cb.n_kinds == 32,
            "ingredients": max(sum(isinstance(k, int) for k in r) for r in cb.recipes.values()) == 5,
            "tasks": len(tm) == 65, "subtasks": max(len(t.subtasks or []) for t in tm.tasks) == 5}[what]
    with pytest.raises(ValueError):
        compile_config(world_params("craft_medium_12x12"), cb, tm, T_MAX)


def check_create_refusals(cpu, capfd):
    """craft_sim_create on a craft_config_t set one past each limit directly: CRAFT_EINVAL, no
    handle, and craft_host.h's message."""
    L = N.lib(cpu=cpu)

    def limits_config():
        return compile_config(world_params("craft_medium_12x12"), Cookbook(yaml_paths("limits")["recipes"]),
                              TaskManager(yaml_paths("limits")["hints"]), T_MAX)

    def kinds(c):
        c.n_kinds = N.MAX_KINDS + 1
        c.n_features = 19 * c.n_kinds + 5

    def recipes(c):
        c.n_recipes = N.MAX_RECIPES + 1

    def ingredients(c):
        c.recipe[N.MAX_RECIPES - 1].n_inputs = N.MAX_INGREDIENTS + 1

    def tasks(c):
        c.n_tasks = N.MAX_TASKS + 1

    def subtasks(c):
        c.task[N.MAX_TASKS - 1].n_subtasks = N.MAX_SUBTASKS + 1

    for change, message in ((None, None), (kinds, "n_kinds out of range"), (recipes, "n_recipes out of range"),
                            (ingredients, "bad recipe"), (tasks, "n_tasks out of range"), (subtasks, "bad task")):
        cfg = limits_config()
        if change:
            change(cfg)
        handle = ctypes.c_void_p()
        capfd.readouterr()
        rc = L.craft_sim_create(ctypes.byref(cfg), 0, 4, 0, 1, ctypes.byref(handle))
        err = capfd.readouterr().err
        if change is None:                                   # the limits themselves are accepted
            assert rc == N.OK and handle.value
            L.craft_sim_destroy(handle)
        else:
            assert rc == N.EINVAL and not handle.value, (message, rc)
            assert f"craft_sim_create: {message}\n" in err, (message, err)


def test_create_refuses_one_past_each_limit_cpu(capfd):
    check_create_refusals(True, capfd)


# ---- the episode queue (shared with the GPU file: the oracle has no queue) ----------------------
QUEUE_KINDS = ("stream", "lang_stream", "rollout_stream", "rollout_teach_stream", "rollout_replay")


def queue_case(name, world, n, seed=11):
    """stream_cases.queue_inputs over the cookbook's primitives and its whole get/make list."""
    from tests.stream_cases import T_MAX as Q_T, queue_inputs
    W, H, _, _ = WORLDS[world]
    return queue_inputs(cookbook_world(world), W, n, seed=seed, H=H, tables=cookbook_tables(name, world, Q_T))


def queue_sim(name, world, n, pool, device):
    from tests.episode_summary_cases import make_sim as summary_sim
    from tests.stream_cases import T_MAX as Q_T
    return summary_sim(cookbook_world(world), n, pool, Q_T, device, **yaml_paths(name))


def run_queue(kind, name, world, devices, ring=3):
    """One run of the shared runner of `kind`: simulators a and b on devices[0] and devices[1]
    (b runs the one-tick loop where the runner has one), further ones as `others`.  35 envs for
    the one-tick entry points, 36 for the K-tick ones (fp32 ring slots of odd rows), 35 for those too
    with a ring of one slot."""
    from tests.lang_stream_cases import run_lang_lockstep
    from tests.rollout_replay_cases import draw_tape, pad_rows, run_replay_against_steps
    from tests.rollout_stream_cases import run_rollout_against_steps
    from tests.rollout_teach_stream_cases import run_teach_against_steps
    from tests.stream_cases import T_MAX as Q_T, run_lockstep as run_stream_lockstep
    n = 35 if kind in ("stream", "lang_stream") or ring == 1 else 36
    pool, specs = queue_case(name, world, n)
    assert int(specs[:, 4].max()) >= (60 if name == "limits" else 26)
    a, b, *others = [queue_sim(name, world, n, pool, d) for d in devices]
    if kind == "stream":
        run_stream_lockstep(a, b, specs, False)
    elif kind == "lang_stream":
        run_lang_lockstep(a, b, specs, False)
    elif kind == "rollout_stream":
        run_rollout_against_steps(a, b, specs, False, ring, "alternate", others=others)
    elif kind == "rollout_teach_stream":
        run_teach_against_steps(a, b, specs, False, ring, "bc", others=others)
    else:
        tape = pad_rows(draw_tape(len(specs), 5), Q_T)
        run_replay_against_steps(a, b, specs, tape, False, ring, others=others)


@pytest.mark.parametrize("name,world", [("limits", "w3"), ("even", "w3")])
@pytest.mark.parametrize("kind", QUEUE_KINDS)
def test_queue_runners_cpu(kind, name, world):
    """The runners' own coverage on these queues, on the CPU variant alone."""
    run_queue(kind, name, world, ("cpu", "cpu") if kind in ("stream", "lang_stream") else ("cpu", "cpu", "cpu"))


SUMMARY_SEED = {"limits": 3, "even": 6}      # of the drawn policy: each meets the pass's conditions below


def check_summary(oracle_mod, device, name="limits", world="w3", n=35, policy_seed=None):
    """craft_episode_summary with distance_out over a pass of 3n + 17 episodes on the cookbook_case
    pool (hand-built rows included) against the copy of the host loop and the oracle
    (episode_summary_cases.check_pass); some get of a kind without a table slot fails with its
    target on the grid, so the second launch's BFS runs for that reason.  Returns the records and
    the outputs."""
    import tests.episode_summary_cases as S
    from tests.stream_cases import T_MAX as Q_T
    case = cookbook_case(oracle_mod, name, world, n=3 * n + 17, max_timesteps=Q_T)
    specs = np.ascontiguousarray(np.stack(case.specs, 1).astype(np.int32))
    sim, probe = (S.make_sim(case.params, n, case.pool, Q_T, device, **case.kw) for _ in range(2))
    r = S.stream_pass(sim, specs, S.drawn_policy(sim, SUMMARY_SEED[name] if policy_seed is None else policy_seed))
    got, want = S.check_pass(oracle_mod, sim, probe, case.pool, specs, r, len(specs), name)
    kinds = np.asarray([case.cfg.task[int(t)].arg_kind for t in specs[:, 4]])
    failed = want["is_get"] & (want["success"] == 0)
    if name == "limits":
        assert (failed & np.isin(kinds, case.no_slot) & (want["distance"] > 0)).any(), "no failed get of a no-slot kind"
        assert (failed & (kinds == 31)).any() and (specs[:, 4] >= 60).any()
    assert (failed & (want["distance"] > 0)).any() and (want["success"] == 1).any()
    return case, specs, S.host(r), got


@pytest.mark.parametrize("kind", ["rollout_stream", "rollout_teach_stream", "rollout_replay"])
def test_queue_runners_ring_of_one_cpu(kind):
    run_queue(kind, "limits", "w3", ("cpu", "cpu", "cpu"), ring=1)


@pytest.mark.parametrize("name", ["limits", "even"])
def test_summary_cpu(oracle_mod, name):
    check_summary(oracle_mod, "cpu", name)


def test_tile_fits_never_undercounts_the_carve():
    """craft_checks.h tile_fits restates the one-tick LDS carve (craft_device.h lds_layout plus the
    teacher tick's subtask bytes) by hand; the HIP library's host-side hook compares the two over
    every tile, grid size, window and kind count of the ABI: no tile the rule admits exceeds a
    workgroup's LDS, and the carve never exceeds the rule's bound."""
    L = N.lib()
    L.craft_debug_tile_fits_drift.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    L.craft_debug_tile_fits_drift.restype = ctypes.c_int
    checked = ctypes.c_int64(0)
    assert L.craft_debug_tile_fits_drift(ctypes.byref(checked)) == 0
    assert checked.value == 3 * 248 * 3 * 31
