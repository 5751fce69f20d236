"""craft_step_lang on the card (the tile kernel's language mode, craft_tile.h MODE_LANG): in
lockstep with the CPU variant of the same ABI (itself checked against the oracle and the
reference's trainers by tests/test_language_rollout_cpu.py), against the composition of the
existing HIP entry points, and the reference's three language trainers' do_rollout through
do_language_rollout."""
import numpy as np
import pytest
import torch

from psketch_amd import _native as N
from psketch_amd import sample_scenarios, synthetic_specs
from tests.helpers import make_tables, row_ids
from tests.language_rollout_cases import (CASES, CASE_IDS, check_case, check_teacher_raise_of_ended_slot,
                                          make_sim)
from tests.test_cpu_variant import cpu_sim
from tests.test_gpu_parity import host, sim_with_pool
from tests.test_language_rollout_cpu import lang_buffers

pytestmark = pytest.mark.gpu

W12, W12_5 = "craft_medium_12x12", "craft_medium_12x12_w5"
W15_7 = dict(WIDTH=15, HEIGHT=15, WINDOW_WIDTH=7, WINDOW_HEIGHT=7, N_WORKSHOPS=3, N_PRIMITIVES=2,
             N_WORLDS=100)
W8 = "craft_medium"
W13_5 = dict(WIDTH=13, HEIGHT=13, WINDOW_WIDTH=5, WINDOW_HEIGHT=5, N_WORKSHOPS=3, N_PRIMITIVES=2,
             N_WORLDS=100)
OUTPUTS = ("obs", "done", "success", "action_record", "ask_record", "transition_code", "labels")


# n: 200 = three full 64-env tiles and one of 8 (3x3 windows); 72 = two 32-env tiles and 8 (5x5);
# lanes / table: craft_sim_tune_teach's knobs (0 = default: quads on 64-env tiles, pairs on 32);
# teach False: label_out NULL, the teacher-less launch
# tile: craft_sim_tune's tile_envs on the HIP side (0 = default: 64 at 3x3, 32 for wider windows)
LANG_ROWS = [
    (W12, 12, 200, 0, 0, True, "f32", 0),
    (W12, 12, 200, 1, 2, True, "f32", 0),
    (W12, 12, 200, 2, 0, True, "bf16", 0),
    (W12, 12, 200, 4, 2, True, "u8", 0),
    (W12, 12, 200, 0, 0, False, "f32", 0),
    (W12_5, 12, 72, 1, 0, True, "f32", 0),
    (W12_5, 12, 72, 2, 2, True, "f32", 0),
    (W12_5, 12, 72, 4, 0, True, "bf16", 0),
    (W12_5, 12, 72, 0, 0, False, "u8", 0),
    (W15_7, 15, 40, 0, 0, True, "f32", 0),
    (W15_7, 15, 40, 1, 2, True, "f32", 0),
    (W15_7, 15, 40, 0, 0, False, "f32", 0),
    (W8, 8, 70, 0, 0, True, "f32", 0),            # 8x8: 2 words per cell set; a 64-env tile and one of 6
    (W13_5, 13, 40, 0, 0, True, "f32", 0),        # 13x13: 5 words; a 32-env tile and one of 8
    (W12_5, 12, 72, 0, 0, True, "f32", 64),       # the 64-env teacher tile on a wide window: quads,
    (W12_5, 12, 72, 2, 0, True, "f32", 64),       # pairs
    (W12, 12, 72, 0, 0, False, "f32", 16),        # the bare tick on 16- and 64-env tiles
    (W12_5, 12, 72, 0, 0, False, "f32", 16),
    (W12_5, 12, 72, 0, 0, False, "f32", 64)]


@pytest.mark.parametrize("world,W,n,lanes,table,teach,fmt,tile", LANG_ROWS, ids=row_ids(LANG_ROWS, 7, ("tile",)))
def test_step_lang_hip_equals_cpu_variant(world, W, n, lanes, table, teach, fmt, tile):
    lang_lockstep(world, W, n, lanes, table, teach, fmt, tile)


def lang_lockstep(world, W, n, lanes, table, teach, fmt, tile, H=None):
    """One LANG_ROWS row (H: the world's height where it is not W)."""
    T, ticks = 12, 14
    params, cb, tm, cfg = make_tables(world, T)
    pool, _, _ = sample_scenarios(params, cb, 123, 24)
    specs = synthetic_specs(pool, W, W if H is None else H, n, 0, seed=6, task_ids=[t.id for t in tm.dataset_tasks()])
    g, c = sim_with_pool(world, n, pool, max_timesteps=T), cpu_sim(world, n, pool, max_timesteps=T)
    g.tune_teach(1, lanes, table)
    if tile:
        g.tune(tile_envs=tile, obs_store=2)      # (2: the store policy of an untuned handle)
    for s in (g, c):
        s.set_obs_format(fmt)
        s.reset(*specs)
    rng = np.random.RandomState(3)
    for t in range(ticks):
        acts = rng.choice(6, size=n, p=[.17, .17, .17, .17, .29, .03]).astype(np.int32)
        alt = rng.randint(0, 6, size=n).astype(np.int32)
        use = (rng.rand(n) < 0.4).astype(np.uint8)
        og, oc = lang_buffers(g, "cuda"), lang_buffers(c)
        if not teach:
            og["labels"] = oc["labels"] = None
        if t % 5 == 4:                           # the hashed draw and no ASK bits
            g.step_lang(None, seed=9, tick=t, **og)
            c.step_lang(None, seed=9, tick=t, **oc)
        else:
            g.step_lang(torch.as_tensor(acts, device="cuda"), tick=t,
                        alt_actions=torch.as_tensor(alt, device="cuda"),
                        use_alt=torch.as_tensor(use, device="cuda"), **og)
            c.step_lang(torch.as_tensor(acts), tick=t, alt_actions=torch.as_tensor(alt),
                        use_alt=torch.as_tensor(use), **oc)
        for k in OUTPUTS + ("any_live",):
            if og[k] is not None:
                assert torch.equal(og[k].cpu(), oc[k]), (k, t)
    assert bool((oc["done"] == 1).all())         # the last ticks ran on all-frozen envs
    sg, sc = g.get_state(), c.get_state()
    for k in sg:
        assert torch.equal(sg[k].cpu(), sc[k]), k
    np.testing.assert_array_equal(host(g.stats()), host(c.stats()))
    g.check()
    c.check()


def test_step_lang_equals_transition_observe_teacher():
    """One launch against the pieces it fuses: craft_transition, the protocol's bookkeeping
    on the host, craft_observe, craft_teacher."""
    world, n, T, ticks = W12, 200, 12, 13
    params, cb, tm, cfg = make_tables(world, T)
    pool, _, _ = sample_scenarios(params, cb, 123, 24)
    specs = synthetic_specs(pool, 12, 12, n, 0, seed=8, task_ids=[t.id for t in tm.dataset_tasks()])
    a, b = sim_with_pool(world, n, pool, max_timesteps=T), sim_with_pool(world, n, pool, max_timesteps=T)
    a.reset(*specs)
    b.reset(*specs)
    rng = np.random.RandomState(4)
    timer = np.full(n, T)
    frozen = np.zeros(n, bool)
    codes = torch.empty(n, dtype=torch.int8, device="cuda")
    obs = b.empty_obs()
    sat = torch.empty(n, dtype=torch.int8, device="cuda")
    for t in range(ticks):
        acts = rng.choice(6, size=n, p=[.17, .17, .17, .17, .29, .03]).astype(np.int32)
        out = lang_buffers(a, "cuda")
        a.step_lang(torch.as_tensor(acts, device="cuda"), tick=t, **out)
        was = frozen.copy()
        b.transition(torch.as_tensor(np.where(was, -1, acts).astype(np.int32), device="cuda"), codes=codes)
        timer[~was] -= 1
        frozen |= ~was & ((acts == N.STOP) | (timer <= 0))
        b.observe(obs=obs, sat=sat)
        labels, _ = b.teacher()
        assert torch.equal(out["obs"], obs), t
        assert torch.equal(out["transition_code"], codes), t
        np.testing.assert_array_equal(host(out["done"]), frozen.astype(np.uint8))
        np.testing.assert_array_equal(host(out["success"]), np.where(frozen, host(sat), -1))
        np.testing.assert_array_equal(host(out["action_record"]), np.where(was, -1, acts))
        np.testing.assert_array_equal(host(out["labels"])[~frozen], host(labels)[~frozen])
        assert (host(out["labels"])[was] == -1).all()
        assert int(out["any_live"][0]) == int((~frozen).any())
    assert frozen.all()
    sa, sb = a.get_state(), b.get_state()
    for k in ("inventory", "grid", "spec"):
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(sa["agent"][:, :3], sb["agent"][:, :3])
    a.check()
    b.check()


@pytest.fixture(scope="module")
def fx(golden):
    return golden("language_rollout.npz")


@pytest.mark.parametrize("mode,is_eval,T", CASES, ids=CASE_IDS)
def test_language_rollout_gpu_vs_reference(fx, mode, is_eval, T):
    check_case(fx, make_sim(fx, T, 0), mode, is_eval, T)


def test_slot_ended_by_step_lang_is_frozen_until_reset():
    world, n = W12, 70
    params, cb, tm, cfg = make_tables(world, 3)
    pool, _, _ = sample_scenarios(params, cb, 123, 8)
    specs = synthetic_specs(pool, 12, 12, n, 0, seed=2, task_ids=[t.id for t in tm.dataset_tasks()])
    sim = sim_with_pool(world, n, pool, max_timesteps=3)
    sim.reset(*specs)
    acts = torch.zeros(n, dtype=torch.int32, device="cuda")
    acts[::2] = N.STOP
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    sim.step_lang(acts, done=done)
    assert host(done).tolist() == [1, 0] * (n // 2)
    before = sim.get_state()
    d2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rec = torch.zeros(n, dtype=torch.int32, device="cuda")
    lab = torch.zeros(n, dtype=torch.int32, device="cuda")
    sim.step(torch.ones(n, dtype=torch.int32, device="cuda"), autoreset=False, done=d2,
             action_record=rec, labels=lab)
    assert bool((d2[::2] == 1).all()) and bool((rec[::2] == -1).all()) and bool((rec[1::2] == 1).all())
    assert bool((lab[::2] == -1).all()) and bool((lab[1::2] >= 0).all())
    after = sim.get_state()
    assert torch.equal(after["agent"][::2], before["agent"][::2])
    assert bool((sim.teacher()[0][::2] == -1).all())
    sim.reset(*specs)                             # craft_reset revives them
    sim.step_lang(acts, done=done, action_record=rec)
    assert torch.equal(rec, acts)
    sim.check()


# table 2: the go leaf is a deferred BFS (the dense pass reports the raise); table 0: the teacher
# table's answer does; one lane and the default quads
@pytest.mark.parametrize("lanes,table", [(0, 0), (0, 2), (1, 2), (2, 0)])
def test_step_lang_teacher_raise_latches_only_for_running_slots(lanes, table):
    check_teacher_raise_of_ended_slot(0, kernel=1, lanes=lanes, table=table)


def test_step_lang_capture_right_after_pool_load():
    """Under stream capture craft_step_lang with labels refuses to build pending teacher-table
    rows (CRAFT_EINVAL), as craft_step_teach does; after sync_table the captured launch replays
    equal to an eager one.  Without labels the launch reads no table and captures at once."""
    world, n = W12, 200
    params, cb, tm, cfg = make_tables(world)
    pool, _, _ = sample_scenarios(params, cb, 123, 24)
    specs = synthetic_specs(pool, 12, 12, n, 0, seed=5, task_ids=[t.id for t in tm.dataset_tasks()])
    a, b = sim_with_pool(world, n, pool), sim_with_pool(world, n, pool)
    a.reset(*specs)
    b.reset(*specs)
    oa, ob = lang_buffers(a, "cuda"), lang_buffers(b, "cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(N.CraftError, match="sync_table") as e:
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                a.step_lang(None, seed=4, tick=0, **oa)
    assert e.value.status == N.EINVAL
    torch.cuda.synchronize()
    a.sync_table()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g2, stream=s):
            a.step_lang(None, seed=4, tick=0, **oa)
    g2.replay()
    torch.cuda.synchronize()
    b.step_lang(None, seed=4, tick=0, **ob)
    for k in OUTPUTS:
        assert torch.equal(oa[k], ob[k]), k
    a.check()
    b.check()
    c = sim_with_pool(world, n, pool)             # pending rows, but no teacher in the launch
    c.reset(*specs)
    oc = lang_buffers(c, "cuda")
    oc["labels"] = None
    g3 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g3, stream=s):
            c.step_lang(None, seed=4, tick=0, **oc)
    g3.replay()
    torch.cuda.synchronize()
    for k in OUTPUTS[:-1]:
        assert torch.equal(oc[k], ob[k]), k
    c.check()
