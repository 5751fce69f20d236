"""Worlds with WIDTH != HEIGHT on the CPU: the oracle, its numpy restatement, the scenario
generators and the CPU variant of the C ABI against the reference's own results on rectangles
(tests/golden/rect_worlds.npz, written by `python tests/golden/make_golden.py rect`), then the CPU
variant against the oracle on every shape of tests/helpers.py RECT_SHAPES.  Every other world of the
suite is square, where a WIDTH written for a HEIGHT changes nothing; tests/test_gpu_rect_worlds.py
runs the HIP kernels on the same shapes."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from psketch_amd import CraftSim, sample_scenarios
from psketch_amd import _native as N
from psketch_amd.cookbook import Task, generator_primitives
from tests.helpers import RECT_FIXTURE_TAGS, RECT_SHAPES, rect_tables, rect_world
from tests.rect_cases import (FORMATS, TeacherCoverage, check_teacher_latch, host, make_sim, oracle_envs,
                              oracle_labels, rect_case, run_lockstep)
from tests.stream_cases import T_MAX, check_against_composition, queue_inputs
from tests.test_cpu_variant import cpu_sim
from tests.test_gpu_parity import set_states
from tests.test_language_rollout_cpu import lang_buffers

TAGS = list(RECT_SHAPES)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rect_worlds.npz")


def test_shapes_are_what_their_rows_say():
    for tag, (W, H, window, prims) in RECT_SHAPES.items():
        assert W != H and 3 <= W <= 16 and 3 <= H <= 16 and tag == f"r{W}x{H}"
    band = {t: (RECT_SHAPES[t][0] - 2) * RECT_SHAPES[t][1] for t in TAGS}
    assert (band["r6x16"], band["r10x16"], band["r12x16"]) == (64, 128, 160)       # full 32-bit words
    assert 4 * 15 * 16 <= 1000 < 4 * 16 * 16 and (7 * 13) % 4 != 0
    assert all(RECT_SHAPES[t][2] > min(RECT_SHAPES[t][:2]) for t in ("r5x16", "r16x5"))


# ---- the oracle and its numpy restatement against the reference ---------------------------------
@pytest.mark.parametrize("tag", RECT_FIXTURE_TAGS)
def test_oracle_and_numpy_random_step_kats(fx, oracle_mod, tag):
    from oracle.craft_numpy import NumpyWorld
    W, H, _, _ = RECT_SHAPES[tag]
    _, _, tm, cfg = rect_tables(tag)
    o, w = oracle_mod.Oracle(cfg), NumpyWorld(cfg)
    p = f"{tag}_kat_"
    assert fx[p + "pre_grid"].shape[1] == W * H and fx[p + "features"].shape[1] == cfg.n_features
    for i in range(len(fx[p + "action"])):
        x, y, d = (int(v) for v in fx[p + "pre_agent"][i])
        a = int(fx[p + "action"][i])
        env = o.env(fx[p + "pre_grid"][i], x, y, d, fx[p + "pre_inv"][i])
        st = {"grid": w.onehot(fx[p + "pre_grid"][i]), "inv": fx[p + "pre_inv"][i].astype(np.float64),
              "pos": (x, y), "dir": d}
        np.testing.assert_array_equal(o.features(env), fx[p + "features"][i], err_msg=str(i))
        np.testing.assert_array_equal(w.features(st), fx[p + "features"][i], err_msg=str(i))
        assert [o.satisfies(env, t) for t in range(len(tm))] == fx[p + "satisfies"][i].tolist(), i
        sat = [w.satisfies(st, t) for t in range(len(tm))]
        assert [-1 if s is None else int(s) for s in sat] == fx[p + "satisfies"][i].tolist(), i
        assert o.step(env, a) == 0
        assert [int(env["x"][0]), int(env["y"][0]), int(env["dir"][0])] == fx[p + "post_agent"][i].tolist(), i
        assert env["inv"][0, :cfg.n_kinds].tolist() == fx[p + "post_inv"][i].tolist(), i
        assert env["grid"][0, :W * H].tolist() == fx[p + "post_grid"][i].tolist(), i
        st2 = w.step(st, a)
        assert list(st2["pos"]) + [st2["dir"]] == fx[p + "post_agent"][i].tolist(), i
        assert st2["inv"].tolist() == fx[p + "post_inv"][i].tolist(), i
        assert st2["grid"].argmax(axis=2).reshape(-1).tolist() == fx[p + "post_grid"][i].tolist(), i


@pytest.mark.parametrize("tag", RECT_FIXTURE_TAGS)
def test_oracle_teacher(fx, oracle_mod, tag):
    _, _, tm, cfg = rect_tables(tag)
    o = oracle_mod.Oracle(cfg)
    p = f"{tag}_teacher_"
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


@pytest.mark.parametrize("tag", RECT_FIXTURE_TAGS)
def test_oracle_and_numpy_rollout(fx, oracle_mod, tag):
    from oracle.craft_numpy import NumpyWorld
    W, H, _, _ = RECT_SHAPES[tag]
    _, _, tm, cfg = rect_tables(tag)
    p = f"{tag}_rollout_"
    o = oracle_mod.Oracle(cfg, fx[p + "pool"])
    sp = fx[p + "spec"]
    envs = o.init_envs(sp[:, 0], sp[:, 1], sp[:, 2], sp[:, 3], sp[:, 4])
    w = NumpyWorld(cfg)
    batch = w.start([w.onehot(g) for g in fx[p + "pool"]], sp)
    seed = int(fx[p + "seed"][0])
    assert fx[p + "obs_ticks"].tolist() == list(range(fx[p + "done"].shape[0]))       # every tick's obs
    assert fx[p + "done"].shape[0] > cfg.max_timesteps                                # timeouts occur
    for t in range(fx[p + "done"].shape[0]):
        rc, obs, reward, done, success = o.batch_tick(envs, 0, None, seed, t, True)
        assert rc == 0
        rec = []
        w.tick(batch, 0, seed, t, rec)
        for got in ((obs, reward, done, success), rec[0]):
            np.testing.assert_array_equal(got[0], fx[p + "obs"][t], err_msg=f"obs t={t}")
            np.testing.assert_array_equal(got[1], fx[p + "reward"][t])
            np.testing.assert_array_equal(got[2], fx[p + "done"][t])
            np.testing.assert_array_equal(got[3], fx[p + "success"][t])
        np.testing.assert_array_equal(np.stack([envs["x"], envs["y"], envs["dir"], envs["timer"]], 1),
                                      fx[p + "agent"][t])
        np.testing.assert_array_equal(envs["inv"][:, :cfg.n_kinds], fx[p + "inv"][t])
        np.testing.assert_array_equal(envs["grid"][:, :W * H], fx[p + "grid"][t])
        np.testing.assert_array_equal(np.asarray([s["pos"] for s in batch["states"]]), fx[p + "agent"][t][:, :2])


# ---- the scenario generators against the reference ----------------------------------------------
@pytest.mark.parametrize("tag", RECT_FIXTURE_TAGS)
def test_scenario_generators_reproduce_reference_stream(fx, oracle_mod, tag):
    """make_data.sample_scenario from RandomState(123) with the duplicate check: the native
    generator (craft_sample_scenarios), the C oracle's mt19937 mode and oracle/make_data_oracle.py
    give the reference's grids, initial positions and MT19937 state after the last draw."""
    from oracle import make_data_oracle
    W, H, _, prims = RECT_SHAPES[tag]
    params, cb, _, _ = rect_tables(tag)
    p = f"{tag}_scen_"
    count = len(fx[p + "grids"])
    ws = [cb.index["workshop%d" % i] for i in range(3)]
    native = sample_scenarios(params, cb, 123, count)
    c_oracle = oracle_mod.generate_scenarios(W, H, cb.index["boundary"], generator_primitives(cb), prims, ws, count,
                                             123, rng="mt19937", dedup=True)
    for grids, init, mt in (native, c_oracle):
        np.testing.assert_array_equal(grids, fx[p + "grids"])
        np.testing.assert_array_equal(init, fx[p + "init"])
        assert np.array_equal(mt[:624], fx[p + "mt_key"]) and mt[624] == fx[p + "mt_pos"][0]
    worlds, inits, rs = make_data_oracle.sample_worlds(params, cb, generator_primitives(cb), 123, count)
    np.testing.assert_array_equal(np.stack([g.reshape(-1) for g in worlds]), fx[p + "grids"])
    np.testing.assert_array_equal(np.asarray(inits), fx[p + "init"])
    st = rs.get_state()
    assert np.array_equal(np.asarray(st[1], dtype=np.uint32), fx[p + "mt_key"]) and st[2] == fx[p + "mt_pos"][0]


# ---- the CPU variant against the reference ------------------------------------------------------
@pytest.mark.parametrize("tag", RECT_FIXTURE_TAGS)
def test_random_step_kats_cpu(fx, tag):
    check_kats(fx, tag, "cpu")


def check_kats(fx, tag, device, world=None, **kw):
    """craft_set_state / craft_observe / craft_transition / craft_get_state on slot lists against
    the reference's features, satisfies and step of the fixture's random states (world: the
    params of the fixture part `tag`, default RECT_SHAPES[tag]'s; kw: CraftSim's recipes, hints)."""
    p = f"{tag}_kat_"
    n = len(fx[p + "action"])
    dev = "cpu" if device == "cpu" else "cuda"
    sim = CraftSim(world or rect_world(*RECT_SHAPES[tag]), n_envs=2 * n + 8, device=device, pool_capacity=n, **kw)
    sim.load_pool(fx[p + "pre_grid"])
    # the states go to the slots 2n+7 .. n+8 (a slot list, in reverse), the results to 0 .. n-1
    slots = torch.arange(2 * n + 7, n + 7, -1, dtype=torch.int32, device=dev)
    agent = fx[p + "pre_agent"].astype(np.int32)
    spec = np.stack([np.arange(n), agent[:, 0], agent[:, 1], agent[:, 2], np.zeros(n)], 1).astype(np.int32)
    sim.set_state(spec, np.concatenate([agent, np.full((n, 1), 40)], 1).astype(np.int32),
                  fx[p + "pre_inv"][:, :sim.n_kinds].astype(np.int32), slots=slots)
    obs = sim.empty_obs(n)
    sim.observe(slots=slots, obs=obs, n=n)
    np.testing.assert_array_equal(host(obs), fx[p + "features"].astype(np.float32))
    sat = torch.empty(n, dtype=torch.int8, device=dev)
    for t in range(fx[p + "satisfies"].shape[1]):
        sim.observe(slots=slots, tasks=torch.full((n,), t, dtype=torch.int32, device=dev), sat=sat, n=n)
        np.testing.assert_array_equal(host(sat), fx[p + "satisfies"][:, t], err_msg=f"task {t}")
    dst = torch.arange(n, dtype=torch.int32, device=dev)
    sim.transition(torch.as_tensor(fx[p + "action"].astype(np.int32), device=dev), src=slots, dst=dst)
    st = sim.get_state(slots=dst)
    sim.check()
    np.testing.assert_array_equal(host(st["agent"][:, :3]), fx[p + "post_agent"])
    np.testing.assert_array_equal(host(st["inventory"]), fx[p + "post_inv"][:, :sim.n_kinds])
    np.testing.assert_array_equal(host(st["grid"]), fx[p + "post_grid"])
    before = sim.get_state(slots=slots)                     # the sources are unchanged
    np.testing.assert_array_equal(host(before["grid"]), fx[p + "pre_grid"])
    np.testing.assert_array_equal(host(before["agent"][:, :3]), fx[p + "pre_agent"])


@pytest.mark.parametrize("tag", RECT_FIXTURE_TAGS)
def test_teacher_cpu(fx, tag):
    W, H, window, prims = RECT_SHAPES[tag]
    p = f"{tag}_teacher_"
    n = len(fx[p + "grid"])
    sim = cpu_sim(rect_world(W, H, window, prims), n, fx[p + "grid"])
    set_states(sim, np.arange(n), fx[p + "agent"], fx[p + "inv"])
    plen = torch.empty(n, dtype=torch.int32)
    for t in range(fx[p + "action"].shape[1]):
        a, _ = sim.teacher(tasks=torch.full((n,), t, dtype=torch.int32), path_len_out=plen, n=n)
        np.testing.assert_array_equal(a.numpy(), fx[p + "action"][:, t], err_msg=f"task {t}")
        ref = fx[p + "path_len"][:, t]
        if (ref != -3).all():
            np.testing.assert_array_equal(plen.numpy(), ref, err_msg=f"task {t}")
        check_teacher_latch(sim, fx[p + "action"][:, t])


@pytest.mark.parametrize("tag", RECT_FIXTURE_TAGS)
def test_rollout_fixture_cpu(fx, tag):
    W, H, window, prims = RECT_SHAPES[tag]
    p = f"{tag}_rollout_"
    sp = fx[p + "spec"]
    E = len(sp)
    sim = cpu_sim(rect_world(W, H, window, prims), E, fx[p + "pool"])
    sim.reset(sp[:, 0], sp[:, 1], sp[:, 2], sp[:, 3], sp[:, 4])
    obs = sim.empty_obs()
    rew = torch.empty(E, dtype=torch.float32)
    done = torch.empty(E, dtype=torch.uint8)
    succ = torch.empty(E, dtype=torch.int8)
    seed = int(fx[p + "seed"][0])
    for t in range(fx[p + "done"].shape[0]):
        sim.step(seed=seed, tick=t, obs=obs, reward=rew, done=done, success=succ)
        st = sim.get_state()
        np.testing.assert_array_equal(done.numpy(), fx[p + "done"][t])
        np.testing.assert_array_equal(succ.numpy(), fx[p + "success"][t])
        np.testing.assert_array_equal(rew.numpy(), fx[p + "reward"][t].astype(np.float32))
        np.testing.assert_array_equal(st["agent"].numpy(), fx[p + "agent"][t])
        np.testing.assert_array_equal(st["inventory"].numpy(), fx[p + "inv"][t][:, :sim.n_kinds])
        np.testing.assert_array_equal(st["grid"].numpy(), fx[p + "grid"][t])
        np.testing.assert_array_equal(obs.numpy(), fx[p + "obs"][t].astype(np.float32), err_msg=f"obs t={t}")
    sim.check()


# ---- the CPU variant against the oracle, every shape --------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_lockstep_vs_oracle_cpu(oracle_mod, tag):
    """200 envs, 45 ticks (more than max_timesteps: timeouts and restarts), every tick's
    observation of every env, and craft_teacher of every env at tick 20 and at the end."""
    case = rect_case(oracle_mod, tag)
    run_lockstep(make_sim(case, "cpu"), case, oracle_mod, fmt=FORMATS[TAGS.index(tag) % 3], teacher_at=(20, 44))


_teach_refs = {}


def teach_reference(oracle_mod, tag, mode, n, launches, K, want_obs=False, seed=7, make_case=rect_case,
                    make_watch=None):
    """rollout_oracle.teach_rollout of `launches` launches of K ticks on rect_case(tag) in `mode`
    (policy = hashed draw; label = every env acts on its label, no auto-reset; bc = half the envs
    act on their labels), chaining label_in; computed once per argument set and left unchanged
    (make_case: what builds the case of `tag`, with rect_case's arguments; make_watch(case): a
    further coverage object for rollout_oracle.teach_rollout's watch, checked here).
    Returns the case, the launch arguments, and per launch the oracle's outputs and a copy of its
    envs after it; asserts the teacher conditions of the run (TeacherCoverage)."""
    from oracle import rollout_oracle
    key = (tag, mode, n, launches, K, want_obs, seed, make_case, make_watch)
    if key in _teach_refs:
        return _teach_refs[key]
    case = make_case(oracle_mod, tag, n=n, seed=4, base=1000)
    o, envs = oracle_envs(oracle_mod, case)
    lsrc = mode in ("label", "bc")
    bc = (np.random.RandomState(5).rand(n) < 0.5).astype(np.uint8) if mode == "bc" else None
    src = np.ones(n, bool) if mode == "label" else (bc.astype(bool) if bc is not None else None)
    a = NS(seed=seed, autoreset=mode != "label", bc=bc, label_in=oracle_labels(o, envs) if lsrc else None,
           label_actions=mode == "label")
    cov = TeacherCoverage(case)
    watch = make_watch(case) if make_watch else None
    if lsrc:
        cov.query(envs, a.label_in)
        if watch is not None:
            watch.query(envs, a.label_in)
    label_in, refs = a.label_in, []
    for l in range(launches):
        ref = rollout_oracle.teach_rollout(o, envs, np.arange(case.base, case.base + n), K, seed=seed, tick0=l * K,
                                           autoreset=a.autoreset, label_in=label_in, label_src=src,
                                           want_obs=want_obs, watch=watch)
        cov.values |= set(ref["labels"][ref["labels"] != -1].tolist())
        cov.query(envs, ref["labels"][-1])          # (the states of the launch's last query)
        label_in = ref["labels"][-1] if lsrc else None
        refs.append((ref, envs.copy()))
    a.coverage = cov
    if watch is not None:
        watch.check()
    _teach_refs[key] = (case, o, a, refs)
    return _teach_refs[key]


def check_teach_rollout(sim, case, a, refs, K, coverage=True):
    """craft_rollout_teach on `sim`, one launch of K ticks per entry of refs (teach_reference),
    chaining label_in, launch by launch: labels, action_record, done, success, the observations
    where the reference has them, and the state after each launch.  Returns the outputs."""
    dev, n = sim.device, case.n
    sim.reset(*case.specs)
    label_in = a.label_in
    outs = []
    for l, (ref, envs) in enumerate(refs):
        out = dict(obs=torch.zeros((K, n, sim.n_features), dtype=torch.float32, device=dev),
                   done=torch.zeros((K, n), dtype=torch.uint8, device=dev),
                   success=torch.zeros((K, n), dtype=torch.int8, device=dev),
                   labels=torch.zeros((K, n), dtype=torch.int32, device=dev),
                   action_record=torch.zeros((K, n), dtype=torch.int32, device=dev))
        # the ring slot of tick t is t % K: launches start at multiples of K
        sim.rollout_teach(K, seed=a.seed, tick0=l * K, autoreset=a.autoreset,
                          label_in=None if label_in is None else torch.as_tensor(label_in, device=dev),
                          behavior_clone=None if a.bc is None else torch.as_tensor(a.bc, device=dev),
                          label_actions=a.label_actions, **out)
        for k in ("labels", "action_record", "done", "success"):
            np.testing.assert_array_equal(host(out[k]), ref[k], err_msg=f"{k}, launch {l}")
        if "obs" in ref:
            np.testing.assert_array_equal(host(out["obs"]), ref["obs"], err_msg=f"obs, launch {l}")
        check_teacher_latch(sim, ref["labels"])
        st = sim.get_state()
        np.testing.assert_array_equal(host(st["agent"][:, :3]), np.stack([envs["x"], envs["y"], envs["dir"]], 1))
        np.testing.assert_array_equal(host(st["inventory"]), envs["inv"][:, :sim.n_kinds])
        np.testing.assert_array_equal(host(st["grid"]), envs["grid"][:, :case.C])
        label_in = ref["labels"][-1] if a.label_in is not None else None
        outs.append(out)
    if coverage:
        a.coverage.check()
    return outs


@pytest.mark.parametrize("mode", ["policy", "label", "bc"])
@pytest.mark.parametrize("tag", TAGS)
def test_rollout_teach_cpu_vs_oracle(oracle_mod, tag, mode):
    case, o, a, refs = teach_reference(oracle_mod, tag, mode, n=104, launches=3, K=15, want_obs=True)
    check_teach_rollout(make_sim(case, "cpu"), case, a, refs, K=15)


@pytest.mark.parametrize("tag", TAGS)
def test_pool_generate_and_distances_cpu(oracle_mod, tag):
    check_pool_generate(oracle_mod, tag, "cpu", 40)
    check_distances_vs_oracle(oracle_mod, tag, "cpu")


def check_pool_generate(oracle_mod, tag, device, count):
    """craft_pool_generate against the oracle's splitmix stream: initial positions and grids."""
    W, H, window, prims = RECT_SHAPES[tag]
    sim = CraftSim(rect_world(W, H, window, prims), n_envs=count, device=device, pool_capacity=count + 3)
    init = sim.generate_pool(count, seed=77, first=3, scenario_id0=500, init_pos=True)
    cb = sim.cookbook
    ws = [cb.index["workshop%d" % i] for i in range(3)]
    grids, oinit, _ = oracle_mod.generate_scenarios(W, H, cb.index["boundary"], generator_primitives(cb), prims, ws,
                                                    count, 77, rng="splitmix", scenario_id0=500)
    np.testing.assert_array_equal(host(init), oinit)
    z = np.zeros(count, np.int32)
    sim.reset(np.arange(3, 3 + count, dtype=np.int32), oinit[:, 0], oinit[:, 1], z, z)
    np.testing.assert_array_equal(host(sim.get_state()["grid"]), grids)
    sim.check()
    return sim, grids, oinit


def check_distances_vs_oracle(oracle_mod, tag, device, make_case=rect_case, n=96, T=6, **kw):
    """craft_rollout_distances after a label-mode rollout without auto-reset, against the
    oracle's closest_resource from each env's final pose on its scenario's initial grid
    (trainers/imitation.py:79-91).  Returns the outputs."""
    # (6 ticks: the nearer targets are reached, the farther ones are not)
    case, o, a, refs = teach_reference(oracle_mod, tag, "label", n, 1, T, make_case=make_case)
    envs = refs[0][1]
    sim = make_sim(case, device, **kw)
    rec = check_teach_rollout(sim, case, a, refs, K=T, coverage=False)[0]["action_record"]
    dev = sim.device
    tasks = case.specs[4]
    succ = np.asarray([o.satisfies(envs[i:i + 1], int(tasks[i])) for i in range(n)], dtype=np.int8)
    is_get = np.asarray([case.cfg.task[int(t)].goal == N.GOAL_GET for t in tasks])
    want = np.full(n, -1, dtype=np.int32)
    for i in np.nonzero(is_get)[0]:
        probe = o.env(case.pool[envs["scenario"][i]], envs["x"][i], envs["y"][i], envs["dir"][i])
        rc, _, ln = o.closest_resource(probe, case.cfg.task[int(tasks[i])].arg_kind)
        want[i] = 0 if succ[i] == 1 else -2 if rc else ln
    assert ((succ == 0) & is_get).any() and ((succ == 1) & is_get).any() and (want > 0).any()
    d = torch.empty(n, dtype=torch.int32, device=dev)
    ig = torch.empty(n, dtype=torch.uint8, device=dev)
    na = torch.empty(n, dtype=torch.int32, device=dev)
    fl = torch.empty(2, dtype=torch.int32, device=dev)
    task_t, succ_t = torch.as_tensor(tasks, device=dev), torch.as_tensor(succ, device=dev)
    sim._check(sim._L.craft_rollout_distances(
        sim._h, task_t.data_ptr(), succ_t.data_ptr(), rec.data_ptr(), T, d.data_ptr(), ig.data_ptr(), na.data_ptr(), fl.data_ptr(), sim._stream()),
        "craft_rollout_distances")
    sim.check()
    np.testing.assert_array_equal(host(d), want)
    np.testing.assert_array_equal(host(ig), is_get.astype(np.uint8))
    np.testing.assert_array_equal(host(na), (host(rec) >= 0).sum(axis=0))
    # (flag 1: a failed get whose grid holds no target, -1, or whose targets cannot be reached, -2)
    assert host(fl).tolist() == [0, int(((want < 0) & is_get).any())]
    return [host(x) for x in (d, ig, na, fl)]


# ---- the fused ticks against the entry points they fuse -----------------------------------------
@pytest.mark.parametrize("tag", ["r13x7", "r6x16"])
@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
def test_step_stream_equals_composition_cpu(tag, wrap):
    W, H, window, prims = RECT_SHAPES[tag]
    world, n = rect_world(W, H, window, prims), 40
    pool, specs = queue_inputs(world, W, n, H=H)
    a, b = cpu_sim(world, n, pool, max_timesteps=T_MAX), cpu_sim(world, n, pool, max_timesteps=T_MAX)
    check_against_composition(a, b, specs, wrap)


@pytest.mark.parametrize("tag", ["r13x7", "r6x16"])
def test_step_lang_equals_composition_cpu(oracle_mod, tag):
    """craft_step_lang against craft_transition, the protocol's bookkeeping on the host,
    craft_observe and craft_teacher, as tests/test_gpu_step_lang.py does on the card."""
    T, ticks = 12, 13
    case = rect_case(oracle_mod, tag, n=100, seed=8, max_timesteps=T)
    n = case.n
    a, b = make_sim(case, "cpu"), make_sim(case, "cpu")
    a.reset(*case.specs)
    b.reset(*case.specs)
    rng = np.random.RandomState(4)
    timer = np.full(n, T)
    frozen = np.zeros(n, bool)
    codes = torch.empty(n, dtype=torch.int8)
    obs = b.empty_obs()
    sat = torch.empty(n, dtype=torch.int8)
    for t in range(ticks):
        acts = rng.choice(6, size=n, p=[.17, .17, .17, .17, .29, .03]).astype(np.int32)
        out = lang_buffers(a)
        a.step_lang(torch.as_tensor(acts), tick=t, **out)
        was = frozen.copy()
        b.transition(torch.as_tensor(np.where(was, -1, acts).astype(np.int32)), codes=codes)
        timer[~was] -= 1
        frozen |= ~was & ((acts == N.STOP) | (timer <= 0))
        b.observe(obs=obs, sat=sat)
        labels, _ = b.teacher()
        assert torch.equal(out["obs"], obs), t
        assert torch.equal(out["transition_code"], codes), t
        np.testing.assert_array_equal(out["done"].numpy(), frozen.astype(np.uint8))
        np.testing.assert_array_equal(out["success"].numpy(), np.where(frozen, sat.numpy(), -1))
        np.testing.assert_array_equal(out["action_record"].numpy(), np.where(was, -1, acts))
        np.testing.assert_array_equal(out["labels"].numpy()[~frozen], labels.numpy()[~frozen])
        assert (out["labels"].numpy()[was] == -1).all()
        assert int(out["any_live"][0]) == int((~frozen).any())
    assert frozen.all()
    sa, sb = a.get_state(), b.get_state()
    for k in ("inventory", "grid", "spec"):
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(sa["agent"][:, :3], sb["agent"][:, :3])


# ---- the drop-in CraftWorld ---------------------------------------------------------------------
def test_shim_on_a_rectangle(fx, oracle_mod, tmp_path, monkeypatch):
    """psketch_amd.worlds on r7x13 (the CPU variant): the (W, H) grid, render, neighbors at the
    four borders, and one demonstration replayed state by state against the oracle."""
    from psketch_amd import worlds
    tag = "r7x13"
    W, H, window, prims = RECT_SHAPES[tag]
    (tmp_path / "configs" / "worlds").mkdir(parents=True)
    (tmp_path / "configs" / "worlds" / "r7x13.yaml").write_text(
        "".join(f"{k}: {v}\n" for k, v in rect_world(W, H, window, prims).items()))
    monkeypatch.chdir(tmp_path)
    cfg = NS(recipes="resources/craft/recipes.yaml", world=NS(name="CraftWorld", config=tag),
             student=NS(model=NS()), teacher=NS(name="DemonstrationTeacher"),
             trainer=NS(hints="resources/craft/hints.hierarchy.yaml", max_timesteps=40),
             random=np.random.RandomState(0))
    w = worlds.CraftWorld(cfg, capacity=256, device="cpu", pool_capacity=8)
    assert (w.WIDTH, w.HEIGHT) == (W, H) and cfg.student.model.input_size == w.n_features
    _, cb, tm, ocfg = rect_tables(tag)
    assert w.n_features == ocfg.n_features
    o = oracle_mod.Oracle(ocfg)
    ids = fx[f"{tag}_scen_grids"][0]
    x, y = (int(v) for v in fx[f"{tag}_scen_init"][0])
    K = cb.n_kinds
    onehot = np.zeros((W, H, K))
    for k in range(1, K):
        onehot[..., k] = ids.reshape(W, H) == k
    s0 = w.init_state(onehot, (x, y))
    assert s0.grid_ids.shape == (W, H) and s0.grid.shape == (W, H, K)
    np.testing.assert_array_equal(s0.grid_ids.reshape(-1), ids)
    rows = s0.render()
    assert len(rows) == H and all(len(r) == 2 * W for r in rows)
    assert rows[H - 1 - y][2 * x] == "v"                       # dir 0 = DOWN at (x, y), top row = y = H-1
    assert sorted(s0.neighbors((W - 1, H - 1))) == [(W - 2, H - 1), (W - 1, H - 2)]
    assert sorted(s0.neighbors((0, 0))) == [(0, 1), (1, 0)]
    assert sorted(s0.neighbors((W - 2, H - 2))) == [(W - 3, H - 2), (W - 2, H - 3), (W - 2, H - 1), (W - 1, H - 2)]
    assert s0.neighbors((W - 2, H - 1), worlds.UP) == [] and s0.neighbors((W - 1, 3), worlds.RIGHT) == []
    assert s0.neighbors((H - 2, 3), worlds.RIGHT) == []        # x = 11 > W - 1: outside
    task = tm["make[plank]"]
    env = o.env(ids, x, y, 0)
    state, steps = s0, 0
    while True:
        np.testing.assert_array_equal(state.features(), o.features(env).astype(np.float64))
        np.testing.assert_array_equal(state.make_navigation_grid(),
                                      (env["grid"][0, :W * H].reshape(W, H) > 0).astype(float))
        rc, a = o.teacher(env, task.id)
        assert rc == 0
        if a == N.STOP:
            break
        _, state = state.step(a)
        o.step(env, a)
        steps += 1
        assert state.pos == (int(env["x"][0]), int(env["y"][0])) and state.dir == int(env["dir"][0])
        np.testing.assert_array_equal(state.inventory, env["inv"][0, :K].astype(np.float64))
    assert steps > 3 and state.satisfies(Task("make[plank]")) is True
    wood = cb.index["wood"]
    assert [tuple(map(int, q)) for q in state.find_resource_positions("wood")] == \
        [tuple(q) for q in np.argwhere(env["grid"][0, :W * H].reshape(W, H) == wood)]
    assert s0.pos == (x, y) and not s0.inventory.any()


def test_rectangular_window_is_refused():
    params = rect_world(7, 13, 3)
    params["WINDOW_HEIGHT"] = 5
    with pytest.raises(N.CraftError):
        CraftSim(params, n_envs=4, device="cpu", pool_capacity=1)
