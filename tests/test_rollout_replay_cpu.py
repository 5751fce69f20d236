"""craft_episode_actions and craft_rollout_replay on the CPU variant of the ABI against the loop
of craft_step_stream calls fed the numpy rule's actions; what the shared checks refuse; that the
rows the GPU tests run exercise what they claim; and rollout.replay on the tape."""
import ctypes

import numpy as np
import pytest
import torch

from psketch_amd import _native as N
from psketch_amd import rollout
from tests import rollout_replay_refusal_cases as RC
from tests.refusal_cases import check_row
from tests.rollout_replay_cases import (TAPE_SEEDS, draw_tape, many_clears_case, many_clears_tape, pad_rows,
                                        run_mixed, run_replay_against_steps, timer_rule_case, wrap_epochs_case)
from tests.rollout_stream_cases import LAUNCHES, ROW_IDS, ROWS, W12, row_sims
from tests.stream_cases import T_MAX, queue_inputs
from tests.test_cpu_variant import cpu_sim
from tests.test_rollout_stream_cpu import demo_inputs

ROW_CASES = [(row, seed) for row, seed in zip(ROWS, TAPE_SEEDS)]


def test_both_libraries_export_the_entry_points():
    for path in (N.LIB_PATH, N.CPU_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in ("craft_episode_actions", "craft_rollout_replay"):
            assert hasattr(lib, name), (path, name)
    assert N.lib(cpu=True).craft_abi_version() == 2


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("case", ROW_CASES, ids=ROW_IDS)
def test_rollout_replay_cpu_equals_step_loop_and_meets_coverage(case, wrap):
    """Each row of the GPU table on the CPU variant, 30 ticks in launches of 7, 7, 7, 7, 2: every
    ring slot, get_state(), stats() and check() after every launch, step_now and action_next
    against the numpy rule, and the step loop's outputs meet every coverage condition with the
    row's tape seed."""
    row, seed = case
    specs, (a, b) = row_sims(row, cpu_sim, cpu_sim)
    tape = pad_rows(draw_tape(len(specs), seed), T_MAX)
    loop = run_replay_against_steps(a, b, specs, tape, wrap, row[6])
    if not wrap:
        # under the imitation protocol an episode takes exactly len(row) ticks: every slot is
        # through its 3-4 entries within 24 ticks
        per_slot = np.zeros(a.n_envs, int)
        np.add.at(per_slot, np.arange(len(specs)) % a.n_envs, (tape >= 0).sum(1))
        assert per_slot.max() <= 24 < sum(LAUNCHES)


def test_rollout_replay_many_clears_cpu():
    n, T = 72, 30
    grids, specs, _, wood = many_clears_case(W12, n, T)
    a, b = cpu_sim(W12, n, grids), cpu_sim(W12, n, grids)
    tape = many_clears_tape(n, len(specs), a.config.max_timesteps)
    loop = run_replay_against_steps(a, b, specs, tape, False, 3, coverage=False, ends=False)
    # not vacuous: the slots whose episodes clear four to six cells (an overflowed list) restarted
    stops = (np.stack(loop.acts) == N.STOP).sum(0)
    assert (stops[np.arange(n) % 7 >= 4] >= 2).all()


def test_rollout_replay_mixes_with_the_other_stream_entry_points_cpu():
    n = 72
    pool, specs = queue_inputs(W12, 12, n)
    a, b = (cpu_sim(W12, n, pool, max_timesteps=T_MAX) for _ in range(2))
    run_mixed(a, b, specs, pad_rows(draw_tape(len(specs), 21), T_MAX))


def test_rollout_replay_timer_rule_cpu():
    n = 40
    pool, specs = queue_inputs(W12, 12, n)
    rows = draw_tape(len(specs), 21)
    rows[2] = np.asarray([0, 1, 2, 3, 4, 0], dtype=np.int32)
    a, b = (cpu_sim(W12, n, pool, max_timesteps=T_MAX) for _ in range(2))
    timer_rule_case(a, b, specs, pad_rows(rows, T_MAX))


def test_rollout_replay_wrap_epochs_cpu():
    n = 40
    pool, specs = queue_inputs(W12, 12, n)
    wrap_epochs_case(cpu_sim(W12, n, pool, max_timesteps=T_MAX), specs)


@pytest.fixture(scope="module")
def handles():
    return RC.make_replay_handles("cpu")


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_rollout_replay_refuses_cpu(handles, row):
    assert row.message.startswith(row.entry + ": ")
    check_row(handles[row.handle], row)


def test_tape_survives_refused_installs_cpu(handles):
    c = handles["taped"]
    for row in RC.ROWS:
        if row.entry == "craft_episode_actions" and row.handle == "taped":
            check_row(c, row)
    RC.check_tape_survives_refusals(c)


def test_episode_queue_drops_the_tape_cpu():
    RC.check_queue_drops_tape(RC.Ctx("begun", "cpu"))


def test_rollout_replay_no_ticks_is_a_no_op_cpu(handles):
    c = handles["taped"]
    before = c.sim.get_state()
    c.sim.rollout_replay(0)
    for k, v in c.sim.get_state().items():
        assert torch.equal(v, before[k]), k
    c.sim.check()


# ---- rollout.replay on the tape ------------------------------------------------------------------
def counting(sim):
    """Wraps the sim's entry points to count calls."""
    calls = {"set_episode_queue": 0, "set_episode_actions": 0, "rollout_stream": 0, "rollout_replay": 0}
    for name in calls:
        inner = getattr(sim, name)

        def wrapped(*a, _inner=inner, _name=name, **kw):
            calls[_name] += 1
            return _inner(*a, **kw)
        setattr(sim, name, wrapped)
    return calls


def check_replay_runs_on_the_tape(sim, golden, K=5):
    grids, specs, seqs = demo_inputs(golden)
    calls = counting(sim)
    info = rollout.replay(sim, specs, seqs, ticks_per_launch=K)
    assert calls["set_episode_queue"] == 1 and calls["set_episode_actions"] == 1
    assert calls["rollout_stream"] == 0
    assert info.launches == -(-info.ticks // K) == calls["rollout_replay"]
    np.testing.assert_array_equal(info.length, [len(s) for s in seqs])
    assert (info.success == 1).all()
    # the same sequences as one -1 padded array (DemonstrationInfo.action_seqs' layout)
    padded = pad_rows(seqs, sim.config.max_timesteps)
    again = rollout.replay(sim, specs, padded, ticks_per_launch=K)
    for k in ("success", "length", "end_pose", "distances"):
        np.testing.assert_array_equal(getattr(again, k), getattr(info, k), err_msg=k)
    assert (again.ticks, again.launches) == (info.ticks, info.launches)
    gap = padded.copy()
    gap[4, 1] = -1                                       # a -1 inside episode 4's actions
    assert len(seqs[4]) > 2
    with pytest.raises(ValueError, match="episode 4"):
        rollout.replay(sim, specs, torch.as_tensor(gap))


def check_replay_epochs(sim, golden, K=7):
    """epochs=2 on a 2n-entry subset: every (episode, step) pair is seen exactly twice."""
    grids, specs, seqs = demo_inputs(golden)
    m = 2 * sim.n_envs
    specs, seqs = specs[:m], seqs[:m]
    seen = np.zeros((m, max(len(s) for s in seqs)), dtype=np.int32)

    def on_chunk(obs, episode, step, action):
        ep, st, ac = (x.cpu().numpy() for x in (episode, step, action))
        kk, ii = np.nonzero(ac >= 0)
        for k, i in zip(kk, ii):
            assert ac[k, i] == seqs[ep[k, i]][st[k, i]]
        np.add.at(seen, (ep[kk, ii], st[kk, ii]), 1)

    info = rollout.replay(sim, specs, seqs, ticks_per_launch=K, on_chunk=on_chunk, epochs=2)
    length = np.asarray([len(s) for s in seqs])
    valid = np.arange(seen.shape[1])[None] < length[:, None]
    assert (seen[valid] == 2).all() and (seen[~valid] == 0).all()
    np.testing.assert_array_equal(info.length, length)
    with pytest.raises(ValueError):
        rollout.replay(sim, specs[:m - 1], seqs[:m - 1], epochs=2)


def test_replay_runs_on_the_tape_cpu(golden):
    grids, _, _ = demo_inputs(golden)
    check_replay_runs_on_the_tape(cpu_sim("craft_medium", 64, grids), golden)


def test_replay_epochs_cpu(golden):
    grids, _, _ = demo_inputs(golden)
    check_replay_epochs(cpu_sim("craft_medium", 16, grids), golden)
