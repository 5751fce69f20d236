"""craft_rollout_teach_stream on the CPU variant of the ABI (its loop of stream ticks into ring
slots) against the loop of craft_step_stream(label_out) calls of its contract; that the rows the
GPU tests run exercise what they claim; the hint-walk config; the four stream entry points mixed on
one handle; what the shared checks refuse; and rollout.demonstrations on the reference's splits."""
import pytest
import torch

from tests import rollout_teach_stream_refusal_cases as RC
from tests.refusal_cases import check_row, make_handles
from tests.rollout_stream_cases import W12
from tests.rollout_teach_stream_cases import (MODES, ROW_IDS, ROWS, check_demonstrations,
                                              check_demonstrations_time_limit, many_clears_run, row_sims, run_hint_walk,
                                              run_mixed,
                                              run_teach_against_steps)
from tests.stream_cases import T_MAX, queue_inputs
from tests.test_cpu_variant import cpu_sim


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_rollout_teach_stream_cpu_equals_step_loop(row, mode, wrap):
    """30 ticks in launches of 7, 7, 7, 7, 2 against the step_stream loop: every ring slot after
    every launch, then get_state() (spec included), stats() and check(); the mode's coverage
    conditions, from the loop's outputs alone (the same rows, queues and seeds as on the GPU)."""
    specs, (a, b) = row_sims(row, cpu_sim, cpu_sim)
    run_teach_against_steps(a, b, specs, wrap, row[5], mode)


@pytest.mark.parametrize("mode", ["bc", "label"])
def test_rollout_teach_stream_hint_walk_cpu(mode):
    run_hint_walk(cpu_sim, cpu_sim, mode)


def test_rollout_teach_stream_mixes_with_the_other_stream_entry_points_cpu():
    pool, specs = queue_inputs(W12, 12, 72)
    run_mixed(cpu_sim(W12, 72, pool, max_timesteps=T_MAX), cpu_sim(W12, 72, pool, max_timesteps=T_MAX), specs)


def test_many_clears_case_meets_its_conditions_cpu():
    """The table on / off case as the GPU test runs it, on the CPU variant: restarts after four
    and more clears, and a move as a restarted slot's label."""
    many_clears_run(cpu_sim, 1)


@pytest.fixture(scope="module")
def handles():
    return make_handles("cpu", names=RC.HANDLES)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_rollout_teach_stream_refuses_cpu(handles, row):
    assert row.message.startswith("craft_rollout_teach_stream: ")
    check_row(handles[row.handle], row)


def test_rollout_teach_stream_no_ticks_is_a_no_op_cpu(handles):
    c = handles["begun"]
    before = c.sim.get_state()
    c.sim.rollout_teach_stream(0)
    for k, v in c.sim.get_state().items():
        assert torch.equal(v, before[k]), k
    c.sim.check()


@pytest.mark.parametrize("split", ["dev", "test"])
def test_demonstrations_reference_split_cpu(golden, split):
    check_demonstrations(cpu_sim, golden, split)


def test_demonstrations_time_limit_cpu(golden):
    check_demonstrations_time_limit(cpu_sim, golden)
