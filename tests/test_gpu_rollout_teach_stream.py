"""craft_rollout_teach_stream on the card (rollout_teach_kernel's QUEUE instantiations,
craft_rollout_teach.h): against the loop of craft_step_stream(label_out) ticks on the card (another
kernel, tile_kernel's MODE_STREAM with the teacher, itself pinned to the CPU variant by
tests/test_gpu_step_stream.py) and against the CPU variant's craft_rollout_teach_stream; with the
teacher table on and off after reloads; in the hint-walk config; mixed with the other stream entry
points; as a captured graph; at full size; and rollout.demonstrations on the reference's splits."""
import numpy as np
import pytest
import torch

from psketch_amd import _native as N
from tests import rollout_teach_stream_refusal_cases as RC
from tests.refusal_cases import check_row, make_handles
from tests.rollout_stream_cases import W12
from tests.rollout_teach_stream_cases import (MODES, ROW_IDS, ROWS, TEACH_RINGS, assert_same, check_demonstrations,
                                              check_demonstrations_time_limit, many_clears_run, row_sims, run_hint_walk,
                                              run_mixed,
                                              run_teach_against_steps, step_teach_ticks, teach_ring_buffers)
from tests.stream_cases import T_MAX, queue_inputs
from tests.test_cpu_variant import cpu_sim
from tests.test_gpu_parity import sim_with_pool

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_rollout_teach_stream_hip_equals_step_stream_and_cpu_variant(row, mode, wrap):
    """Sim a (HIP) runs rollout_teach_stream, sim b (HIP) the contract's step_stream(labels=) loop
    into the same ring slots, sim c (the CPU variant) rollout_teach_stream: launches of 7, 7, 7,
    7, 2 ticks; after each launch a and c must equal b in every ring slot, get_state(), stats()
    and check().  The mode's coverage, from b's outputs alone, is asserted."""
    specs, (a, b, c) = row_sims(row, sim_with_pool, sim_with_pool, cpu_sim)
    run_teach_against_steps(a, b, specs, wrap, row[5], mode, others=(c,))


def test_rollout_teach_stream_table_on_and_off_after_reloads():
    """Restarts after 0..6 clears onto the other scenario, the teacher table always read and
    never read: each equal to its step_stream loop, and to each other."""
    on, off = many_clears_run(sim_with_pool, 1), many_clears_run(sim_with_pool, 2)
    for k in TEACH_RINGS:
        assert torch.equal(on[k], off[k]), k


@pytest.mark.parametrize("mode", ["bc", "label"])
def test_rollout_teach_stream_hint_walk(mode):
    """A task that keeps the hint walk (the row-synchronous mode) mixed on the queue with
    tabulated ones: restarts both ways, equal to the step loop and to the CPU variant."""
    run_hint_walk(sim_with_pool, sim_with_pool, mode, others=(cpu_sim,))


def test_rollout_teach_stream_mixes_with_the_other_stream_entry_points():
    pool, specs = queue_inputs(W12, 12, 72)
    run_mixed(sim_with_pool(W12, 72, pool, max_timesteps=T_MAX), sim_with_pool(W12, 72, pool, max_timesteps=T_MAX), specs)


def test_rollout_teach_stream_graph_replay():
    """One 8-tick hashed launch on a wrap queue captured after sync_table() and replayed three
    times: equal to three eager launches with the same tick0 on a twin."""
    n, ring = 72, 8
    pool, specs = queue_inputs(W12, 12, n)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes(wrap=True)
        s.sync_table()
    ra, rb = teach_ring_buffers(a, ring), teach_ring_buffers(b, ring)
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            a.rollout_teach_stream(8, seed=5, tick0=0, **ra)
    restarts = 0
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        b.rollout_teach_stream(8, seed=5, tick0=0, **rb)
        assert_same(a, b, ra, rb, f"after replay {r}")
        restarts += int((rb["episode_end"] >= 0).sum())
    assert restarts > n
    # an eager launch after the replays: the eager counter was never touched
    a.rollout_teach_stream(8, seed=2, tick0=0, **ra)
    b.rollout_teach_stream(8, seed=2, tick0=0, **rb)
    assert_same(a, b, ra, rb, "after the eager launch")


def test_rollout_teach_stream_capture_right_after_pool_load():
    """The HIP library's own refusal: a launch captured straight after load_pool, while the new
    rows wait for their teacher-table entries, is refused (they would be rebuilt on every
    replay) and leaves the handle usable for an eager launch."""
    n = 72
    pool, specs = queue_inputs(W12, 12, n)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes(wrap=True)
    ra, rb = teach_ring_buffers(a, 8), teach_ring_buffers(b, 8)
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(N.CraftError, match="sync_table"):
        with torch.cuda.stream(st):
            with torch.cuda.graph(g, stream=st):
                a.rollout_teach_stream(8, seed=5, tick0=0, **ra)
    torch.cuda.synchronize()
    a.rollout_teach_stream(8, seed=5, tick0=0, **ra)
    b.rollout_teach_stream(8, seed=5, tick0=0, **rb)
    assert_same(a, b, ra, rb, "after the refused capture")


@pytest.mark.parametrize("mode", ["hashed", "label"])
def test_rollout_teach_stream_full_size(mode):
    """65,536 + 8 envs (12x12, 3x3 windows, u8 obs, ring 2, 10 ticks): the only size at which a
    workgroup runs a second tile.  Compared on the device against the step_stream loop."""
    n, ring, T = 65536 + 8, 2, 10
    pool, specs = queue_inputs(W12, 12, n, pool_size=64)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    for s in (a, b):
        s.set_obs_format("u8")
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes(wrap=True)
    ra, rb = teach_ring_buffers(a, ring), teach_ring_buffers(b, ring)
    cur = a.teacher()[0].clone()
    a.rollout_teach_stream(T, seed=7, tick0=0, label_in=cur, label_actions=mode == "label", **ra)
    step_teach_ticks(b, rb, ring, 0, T, None, 7, mode, None, cur.clone())
    for k in TEACH_RINGS:
        assert torch.equal(ra[k], rb[k]), k
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.stats(), b.stats())
    assert int(b.stats()[1]) >= n                       # every slot ended an episode (T_MAX < 10)
    a.check()
    b.check()


@pytest.fixture(scope="module")
def handles():
    return make_handles(0, names=RC.HANDLES)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_rollout_teach_stream_refuses_hip(handles, row):
    assert row.message.startswith("craft_rollout_teach_stream: ")
    check_row(handles[row.handle], row)


def test_rollout_teach_stream_no_ticks_is_a_no_op_hip(handles):
    c = handles["begun"]
    before = c.sim.get_state()
    c.sim.rollout_teach_stream(0)
    for k, v in c.sim.get_state().items():
        assert torch.equal(v, before[k]), k
    c.sim.check()


@pytest.mark.parametrize("split", ["dev", "test"])
def test_demonstrations_reference_split_gpu(golden, split):
    """rollout.demonstrations on the card: the fixture's sequences, and the CPU variant's info."""
    from psketch_amd import rollout
    from tests.rollout_teach_stream_cases import demo_split
    gpu = check_demonstrations(sim_with_pool, golden, split)
    grids, specs, _ = demo_split(golden, split)
    cpu = rollout.demonstrations(cpu_sim("craft_medium", 104, grids, max_timesteps=40), specs)
    for k in ("action_seqs", "length", "success", "end_pose"):
        np.testing.assert_array_equal(getattr(gpu, k), getattr(cpu, k), err_msg=k)
    assert gpu.ticks == cpu.ticks


def test_demonstrations_time_limit_gpu(golden):
    check_demonstrations_time_limit(sim_with_pool, golden)
