"""craft_rollout_stream on the card (rollout_split_kernel's QUEUE instantiations,
craft_rollout_split.h): against craft_step_stream on the card tick by tick (another kernel,
tile_kernel's MODE_STREAM, itself pinned to the CPU variant and to the composition of entry points
by tests/test_gpu_step_stream.py) and against the CPU variant's craft_rollout_stream; mixed with the
one-tick stream entry points; restarting after many clears; as a captured graph; and
rollout.replay on the reference's demonstrations."""
import numpy as np
import pytest
import torch

from psketch_amd import _native as N
from psketch_amd import rollout
from tests import rollout_stream_refusal_cases as RC
from tests.refusal_cases import check_row, make_handles
from tests.rollout_stream_cases import (ROW_IDS, ROWS, W12, assert_same, many_clears_case, ring_buffers,
                                        row_sims, run_rollout_against_steps, step_ticks)
from tests.stream_cases import T_MAX, draw_actions, queue_inputs
from tests.test_cpu_variant import cpu_sim
from tests.test_gpu_parity import sim_with_pool
from tests.test_rollout_stream_cpu import check_replay, demo_inputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_rollout_stream_hip_equals_step_stream_and_cpu_variant(row, wrap):
    """Sim a (HIP) runs rollout_stream, sim b (HIP) step_stream(teach=False) tick by tick into the
    same ring slots, sim c (the CPU variant) rollout_stream: launches of 7, 7, 7, 7, 2 ticks,
    given and hashed actions alternating; after each launch a and c must equal b in every ring
    slot, get_state(), stats() and check().  The coverage, from b's outputs alone, is asserted."""
    specs, (a, b, c) = row_sims(row, sim_with_pool, sim_with_pool, others=(cpu_sim,))
    run_rollout_against_steps(a, b, specs, wrap, row[6], "alternate", others=(c,))


def test_rollout_stream_mixes_with_the_one_tick_entry_points():
    """rollout_stream(5), one step_stream, one step_lang_stream, rollout_stream(5) on sim a; the
    same twelve ticks with the one-tick calls only on sim b: one cursor, everything equal."""
    n, ring = 72, 12
    pool, specs = queue_inputs(W12, 12, n)
    a, b = (sim_with_pool(W12, n, pool, max_timesteps=T_MAX) for _ in range(2))
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes()
    ra, rb = ring_buffers(a, ring), ring_buffers(b, ring)
    rng = np.random.RandomState(6)
    acts = np.stack([draw_actions(rng, n) for _ in range(ring)])
    dacts = torch.as_tensor(acts, device="cuda")
    lang = ("obs", "done", "success", "episode_end", "end_pose", "episode_now")

    a.rollout_stream(5, tick0=0, actions=dacts[:5], **ra)
    step_ticks(a, ra, ring, 5, 1, acts[5:6], 0)
    a.step_lang_stream(dacts[6], tick=6, **{k: ra[k][6] for k in lang})
    a.rollout_stream(5, tick0=7, actions=dacts[7:], **ra)

    step_ticks(b, rb, ring, 0, 6, acts[:6], 0)
    b.step_lang_stream(dacts[6], tick=6, **{k: rb[k][6] for k in lang})
    step_ticks(b, rb, ring, 7, 5, acts[7:], 0)
    assert_same(a, b, ra, rb, "after the twelve ticks")
    end = rb["episode_end"].cpu().numpy()
    assert (end[:5] >= 0).any() and (end[5] >= 0).any() and (end[6] >= 0).any() and (end[7:] >= 0).any()


def test_rollout_stream_restart_after_many_clears():
    """Episodes that clear up to six cells and then STOP onto the other scenario, inside the
    launches, against step_stream: each slot ends on the other scenario's pristine row minus its
    running episode's clears."""
    n, T = 72, 30
    grids, specs, acts, wood = many_clears_case(W12, n, T)
    a, b = sim_with_pool(W12, n, grids), sim_with_pool(W12, n, grids)
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes()
    ra, rb = ring_buffers(a, 3), ring_buffers(b, 3)
    t0 = 0
    moved = np.zeros(n, int)
    for k in (7, 7, 7, 7, 2):
        a.rollout_stream(k, tick0=t0, actions=torch.as_tensor(acts[t0:t0 + k], device="cuda"), **ra)
        for j in range(k):
            step_ticks(b, rb, 3, t0 + j, 1, acts[t0 + j:t0 + j + 1], 0)
            end, now = (rb[x][(t0 + j) % 3].cpu().numpy() for x in ("episode_end", "episode_now"))
            ended = end >= 0
            assert (specs[end[ended], 0] != specs[now[ended], 0]).all()     # onto the other scenario
            moved += ended
        assert_same(a, b, ra, rb, f"after tick {t0 + k - 1}")
        t0 += k
    # not vacuous: the slots whose episodes clear four to six cells (an overflowed list) restarted
    many = np.arange(n) % 7 >= 4
    assert (moved[many] >= 2).all()
    clears_now = np.asarray([([N.USE, N.RIGHT] * (i % 7) + [N.STOP])[:T % (2 * (i % 7) + 1)].count(N.USE)
                             for i in range(n)])
    woods = (a.get_state(fields=("grid",))["grid"].cpu().numpy() == wood).sum(1)
    np.testing.assert_array_equal(woods, 7 - clears_now)


def test_rollout_stream_linear_graph():
    """One rollout_stream(4) launch captured as a linear graph (a memset and a kernel), reading an
    actions buffer updated in place, replayed three times: equal to twelve eager step_stream
    ticks (tick0 and so the ring slots are the capture's: ring 4, slots 0..3 every replay)."""
    n = 72
    pool, specs = queue_inputs(W12, 12, n)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes()
    rng = np.random.RandomState(8)
    acts_host = np.stack([draw_actions(rng, n) for _ in range(12)]).reshape(3, 4, n)
    acts = torch.zeros((4, n), dtype=torch.int32, device="cuda")
    ra, rb = ring_buffers(a, 4), ring_buffers(b, 4)
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            a.rollout_stream(4, tick0=0, actions=acts, **ra)
    restarts = 0
    for r in range(3):
        acts.copy_(torch.as_tensor(acts_host[r]))
        g.replay()
        torch.cuda.synchronize()
        step_ticks(b, rb, 4, 0, 4, acts_host[r], 0)
        assert_same(a, b, ra, rb, f"after replay {r}")
        restarts += int((rb["episode_end"] >= 0).sum())
    assert restarts > n
    # an eager launch after the replays: the eager counter was never touched
    a.rollout_stream(4, tick0=0, seed=2, **ra)
    step_ticks(b, rb, 4, 0, 4, None, 2)
    assert_same(a, b, ra, rb, "after the eager launch")


def test_rollout_stream_empty_and_single_env():
    pool, specs = queue_inputs(W12, 12, 1)
    a, b = sim_with_pool(W12, 1, pool, max_timesteps=T_MAX), sim_with_pool(W12, 1, pool, max_timesteps=T_MAX)
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes(wrap=True)
    ra, rb = ring_buffers(a, 3), ring_buffers(b, 3)
    a.rollout_stream(0, **ra)                           # no ticks: nothing written, nothing moved
    assert_same(a, b, ra, rb, "after no ticks")
    a.rollout_stream(20, seed=4, tick0=0, **ra)
    step_ticks(b, rb, 3, 0, 20, None, 4)
    assert_same(a, b, ra, rb, "one env, 20 ticks")
    a.rollout_stream(3, tick0=20)                       # every output NULL
    step_ticks(b, ring_buffers(b, 3), 3, 20, 3, None, 0)
    assert_same(a, b, ra, rb, "no outputs")
    assert int(b.stats()[1]) >= 3                       # episodes ended and restarted


@pytest.fixture(scope="module")
def handles():
    return make_handles(0, names=RC.HANDLES)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_rollout_stream_refuses_hip(handles, row):
    assert row.message.startswith("craft_rollout_stream: ")
    check_row(handles[row.handle], row)


def test_replay_reference_demonstrations_gpu(golden):
    """The dev split's demonstrations through rollout.replay on the card (256 slots, 32 ticks per
    launch): every episode succeeds in len(actions) ticks, the chunks hold every (state, action)
    pair once, sampled rows equal rebuilt states, and the results equal the CPU run's."""
    grids, specs, seqs = demo_inputs(golden)
    gpu = check_replay(sim_with_pool("craft_medium", 256, grids), sim_with_pool("craft_medium", 50, grids),
                       specs, seqs, 32)
    cpu = rollout.replay(cpu_sim("craft_medium", 64, grids), specs, seqs)
    for k in ("success", "length", "end_pose"):
        np.testing.assert_array_equal(getattr(gpu, k), getattr(cpu, k), err_msg=k)
