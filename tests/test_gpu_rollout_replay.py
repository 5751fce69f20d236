"""craft_episode_actions and craft_rollout_replay on the card (rollout_split_kernel's TAPE
instantiations, craft_rollout_split.h): against craft_step_stream on the card tick by tick, fed
the numpy rule's actions, and against the CPU variant's craft_rollout_replay; mixed with the other
stream entry points; restarting after many clears; the timer rule; epochs under wrap; as a
captured graph; what both entry points refuse; and rollout.replay on the tape."""
import numpy as np
import pytest
import torch

from psketch_amd import _native as N
from tests import rollout_replay_refusal_cases as RC
from tests.refusal_cases import check_row
from tests.rollout_replay_cases import (TAPE_SEEDS, StepLoop, assert_replay_same, begin, draw_tape,
                                        many_clears_case, many_clears_tape, pad_rows, replay_buffers, run_mixed,
                                        run_replay_against_steps, timer_rule_case, wrap_epochs_case)
from tests.rollout_stream_cases import ROW_IDS, ROWS, W12, row_sims
from tests.stream_cases import T_MAX, queue_inputs
from tests.test_cpu_variant import cpu_sim
from tests.test_gpu_parity import sim_with_pool
from tests.test_rollout_replay_cpu import check_replay_epochs, check_replay_runs_on_the_tape
from tests.test_rollout_stream_cpu import demo_inputs

pytestmark = pytest.mark.gpu

ROW_CASES = [(row, seed) for row, seed in zip(ROWS, TAPE_SEEDS)]


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("case", ROW_CASES, ids=ROW_IDS)
def test_rollout_replay_hip_equals_step_stream_and_cpu_variant(case, wrap):
    """Sim a (HIP) runs rollout_replay, sim b (HIP) step_stream tick by tick into the same ring
    slots with the numpy rule's actions, sim c (the CPU variant) rollout_replay: launches of 7, 7,
    7, 7, 2 ticks; after each launch a and c must equal b in every ring slot, get_state(), stats()
    and check(), and their step_now and action_next the numpy rule.  The coverage, from b's
    outputs alone, is asserted."""
    row, seed = case
    specs, (a, b, c) = row_sims(row, sim_with_pool, sim_with_pool, others=(cpu_sim,))
    tape = pad_rows(draw_tape(len(specs), seed), T_MAX)
    run_replay_against_steps(a, b, specs, tape, wrap, row[6], others=(c,))


def test_rollout_replay_restart_after_many_clears():
    """Episodes that clear up to six cells and then STOP onto the other scenario, inside the
    launches, with the script read from the tape."""
    n, T = 72, 30
    grids, specs, _, wood = many_clears_case(W12, n, T)
    a, b = sim_with_pool(W12, n, grids), sim_with_pool(W12, n, grids)
    tape = many_clears_tape(n, len(specs), a.config.max_timesteps)
    loop = run_replay_against_steps(a, b, specs, tape, False, 3, coverage=False, ends=False)
    stops = (np.stack(loop.acts) == N.STOP).sum(0)
    assert (stops[np.arange(n) % 7 >= 4] >= 2).all()
    clears_now = np.asarray([([N.USE, N.RIGHT] * (i % 7) + [N.STOP])[:T % (2 * (i % 7) + 1)].count(N.USE)
                             for i in range(n)])
    woods = (a.get_state(fields=("grid",))["grid"].cpu().numpy() == wood).sum(1)
    np.testing.assert_array_equal(woods, 7 - clears_now)


def test_rollout_replay_mixes_with_the_other_stream_entry_points():
    n = 72
    pool, specs = queue_inputs(W12, 12, n)
    a, b = (sim_with_pool(W12, n, pool, max_timesteps=T_MAX) for _ in range(2))
    run_mixed(a, b, specs, pad_rows(draw_tape(len(specs), 21), T_MAX))


def test_rollout_replay_timer_rule():
    n = 40
    pool, specs = queue_inputs(W12, 12, n)
    rows = draw_tape(len(specs), 21)
    rows[2] = np.asarray([0, 1, 2, 3, 4, 0], dtype=np.int32)
    a, b = (sim_with_pool(W12, n, pool, max_timesteps=T_MAX) for _ in range(2))
    timer_rule_case(a, b, specs, pad_rows(rows, T_MAX), others=(cpu_sim(W12, n, pool, max_timesteps=T_MAX),))


def test_rollout_replay_wrap_epochs():
    n = 72
    pool, specs = queue_inputs(W12, 12, n)
    wrap_epochs_case(sim_with_pool(W12, n, pool, max_timesteps=T_MAX), specs)


def test_rollout_replay_linear_graph():
    """One rollout_replay(4) launch captured as a linear graph (a memset and a kernel, no actions
    buffer), replayed three times: equal to twelve eager step_stream ticks (tick0 and so the ring
    slots are the capture's: ring 4, slots 0..3 every replay); then an eager launch."""
    n = 72
    pool, specs = queue_inputs(W12, 12, n)
    tape = pad_rows(draw_tape(len(specs), 21), T_MAX)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    begin((a, b), specs, tape, True)
    loop = StepLoop(b, tape, 4, T_MAX)
    ra = replay_buffers(a, 4)
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            a.rollout_replay(4, tick0=0, **ra)
    restarts = 0
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        loop.ticks(0, 4)
        assert_replay_same(a, loop, ra, f"after replay {r}")
        restarts += int((loop.rb["episode_end"] >= 0).sum())
    assert restarts > n
    # an eager launch after the replays: the eager counter was never touched
    a.rollout_replay(4, tick0=0, **ra)
    loop.ticks(0, 4)
    assert_replay_same(a, loop, ra, "after the eager launch")


def test_rollout_replay_single_env_and_no_outputs():
    pool, specs = queue_inputs(W12, 12, 1)
    tape = pad_rows(draw_tape(len(specs), 21), T_MAX)
    a, b = sim_with_pool(W12, 1, pool, max_timesteps=T_MAX), sim_with_pool(W12, 1, pool, max_timesteps=T_MAX)
    begin((a, b), specs, tape, True)
    loop = StepLoop(b, tape, 3, T_MAX)
    ra = replay_buffers(a, 3)
    a.rollout_replay(20, tick0=0, **ra)
    loop.ticks(0, 20)
    assert_replay_same(a, loop, ra, "one env, 20 ticks")
    a.rollout_replay(3, tick0=20)                       # every output NULL
    keep = {k: v.clone() for k, v in loop.rb.items()}
    loop.ticks(20, 3)
    loop.rb = keep
    assert_replay_same(a, loop, ra, "no outputs", rows=slice(0, 0))


@pytest.fixture(scope="module")
def handles():
    return RC.make_replay_handles(0)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_rollout_replay_refuses_hip(handles, row):
    assert row.message.startswith(row.entry + ": ")
    check_row(handles[row.handle], row)


def test_tape_survives_refused_installs_hip(handles):
    c = handles["taped"]
    for row in RC.ROWS:
        if row.entry == "craft_episode_actions" and row.handle == "taped":
            check_row(c, row)
    RC.check_tape_survives_refusals(c)


def test_episode_queue_drops_the_tape_hip():
    RC.check_queue_drops_tape(RC.Ctx("begun", 0))


def test_replay_runs_on_the_tape_gpu(golden):
    grids, _, _ = demo_inputs(golden)
    check_replay_runs_on_the_tape(sim_with_pool("craft_medium", 256, grids), golden, K=32)


def test_replay_epochs_gpu(golden):
    grids, _, _ = demo_inputs(golden)
    check_replay_epochs(sim_with_pool("craft_medium", 48, grids), golden)
