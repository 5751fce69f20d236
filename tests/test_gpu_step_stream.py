"""craft_step_stream on the card (the tile kernel's MODE_STREAM, craft_tile.h): in lockstep with
the CPU variant of the same ABI (itself checked by tests/test_stream_cpu.py), against the
composition of the existing HIP entry points, as one captured graph, and rollout.evaluate against
do_rollout and the reference's ImitationTrainer.evaluate."""
import numpy as np
import pytest
import torch

from tests.evaluate_cases import check_evaluate_equals_do_rollout, check_evaluate_equals_reference
from tests.helpers import row_ids
from tests.stream_cases import (STREAM_OUTPUTS, T_MAX, check_against_composition, queue_inputs, run_lockstep,
                                stream_buffers)
from tests.test_cpu_variant import cpu_sim
from tests.test_gpu_parity import sim_with_pool

pytestmark = pytest.mark.gpu

W12, W12_5 = "craft_medium_12x12", "craft_medium_12x12_w5"
W15_7 = dict(WIDTH=15, HEIGHT=15, WINDOW_WIDTH=7, WINDOW_HEIGHT=7, N_WORKSHOPS=3, N_PRIMITIVES=2,
             N_WORLDS=100)
W8 = "craft_medium"
W13_5 = dict(WIDTH=13, HEIGHT=13, WINDOW_WIDTH=5, WINDOW_HEIGHT=5, N_WORKSHOPS=3, N_PRIMITIVES=2,
             N_WORLDS=100)


# n: 200 = three full 64-env tiles and one of 8 (3x3 windows); 72 = two 32-env tiles and 8 (5x5);
# lanes / table: craft_sim_tune_teach's knobs (0 = default: quads on 64-env tiles, pairs on 32);
# teach False: label_out NULL, the teacher-less launch
# tile: craft_sim_tune's tile_envs on the HIP side (0 = default: 64 at 3x3, 32 for wider windows)
STREAM_ROWS = [
    (W12, 12, 200, 0, 0, True, "f32", 0),
    (W12, 12, 200, 1, 2, True, "bf16", 0),
    (W12, 12, 200, 2, 0, True, "u8", 0),
    (W12, 12, 200, 4, 2, True, "f32", 0),
    (W12, 12, 200, 0, 0, False, "f32", 0),
    (W12_5, 12, 72, 1, 0, True, "f32", 0),
    (W12_5, 12, 72, 2, 2, True, "bf16", 0),
    (W12_5, 12, 72, 4, 0, True, "f32", 0),
    (W12_5, 12, 72, 0, 0, False, "u8", 0),
    (W15_7, 15, 40, 0, 0, True, "f32", 0),
    (W15_7, 15, 40, 0, 0, False, "f32", 0),
    (W8, 8, 70, 0, 0, True, "f32", 0),            # 8x8: 2 words per cell set; a 64-env tile and one of 6
    (W13_5, 13, 40, 0, 0, True, "f32", 0),        # 13x13: 5 words; a 32-env tile and one of 8
    (W12_5, 12, 72, 0, 0, True, "f32", 64),       # the 64-env teacher tile on a wide window: quads,
    (W12_5, 12, 72, 2, 0, True, "f32", 64),       # pairs
    (W12, 12, 72, 0, 0, False, "f32", 16),        # the bare tick on 16- and 64-env tiles
    (W12_5, 12, 72, 0, 0, False, "f32", 16),
    (W12_5, 12, 72, 0, 0, False, "f32", 64)]


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("world,W,n,lanes,table,teach,fmt,tile", STREAM_ROWS, ids=row_ids(STREAM_ROWS, 7, ("tile",)))
def test_step_stream_hip_equals_cpu_variant(world, W, n, lanes, table, teach, fmt, tile, wrap):
    stream_lockstep(world, W, n, lanes, table, teach, fmt, tile, wrap)


def stream_lockstep(world, W, n, lanes, table, teach, fmt, tile, wrap, H=None):
    """One STREAM_ROWS row (H: the world's height where it is not W)."""
    pool, specs = queue_inputs(world, W, n, H=H)
    g, c = sim_with_pool(world, n, pool, max_timesteps=T_MAX), cpu_sim(world, n, pool, max_timesteps=T_MAX)
    g.tune_teach(1, lanes, table)
    if tile:
        g.tune(tile_envs=tile, obs_store=2)      # (2: the store policy of an untuned handle)
    for s in (g, c):
        s.set_obs_format(fmt)
    run_lockstep(g, c, specs, wrap, teach=teach)


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
def test_step_stream_equals_step_set_state_observe_teacher(wrap):
    n = 200
    pool, specs = queue_inputs(W12, 12, n)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    check_against_composition(a, b, specs, wrap)


def test_step_stream_linear_graph():
    """Four step_stream launches captured as one linear graph (no parallel branches), reading an
    actions buffer updated in place, replayed three times: equal to twelve eager ticks."""
    n = 200
    pool, specs = queue_inputs(W12, 12, n)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes()
        s.sync_table()
    rng = np.random.RandomState(8)
    acts_host = rng.choice(6, size=(3, 4, n), p=[.18, .18, .18, .18, .18, .10]).astype(np.int32)
    acts = torch.zeros((4, n), dtype=torch.int32, device="cuda")
    outs = [stream_buffers(a) for _ in range(4)]
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            for k in range(4):
                a.step_stream(acts[k], tick=k, **outs[k])
    restarts = 0
    for r in range(3):
        acts.copy_(torch.as_tensor(acts_host[r]))
        for o in outs:
            o["any_live"].zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in range(4):
            ob = stream_buffers(b)
            b.step_stream(torch.as_tensor(acts_host[r, k], device="cuda"), tick=k, **ob)
            for name in STREAM_OUTPUTS + ("any_live",):
                assert torch.equal(outs[k][name], ob[name]), (name, r, k)
            restarts += int((ob["episode_end"] >= 0).sum())
    assert restarts > n
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.stats(), b.stats())
    a.check()
    b.check()


def test_evaluate_equals_do_rollout_gpu(golden):
    check_evaluate_equals_do_rollout(golden, 0)


def test_evaluate_equals_reference_gpu(golden):
    check_evaluate_equals_reference(golden, 0)
