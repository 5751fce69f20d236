"""The episode queue on the CPU variant of the ABI (craft_episode_queue, craft_episode_begin,
craft_step_stream, include/craft.h): the tick against the entry points it fuses, its argument
errors, sharding over handles, and rollout.evaluate against do_rollout and against the
reference's ImitationTrainer.evaluate (tests/golden/imitation_evaluate.npz).
tests/test_gpu_step_stream.py runs the same checks, and HIP against this library, on the card."""
import ctypes

import numpy as np
import pytest
import torch

from psketch_amd import _native as N
from tests.evaluate_cases import check_evaluate_equals_do_rollout, check_evaluate_equals_reference
from tests.stream_cases import T_MAX, check_against_composition, queue_inputs, stream_buffers
from tests.test_cpu_variant import cpu_sim

W12 = "craft_medium_12x12"


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
def test_step_stream_equals_step_set_state_observe_teacher_cpu(wrap):
    n = 40
    pool, specs = queue_inputs(W12, 12, n)
    a, b = cpu_sim(W12, n, pool, max_timesteps=T_MAX), cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    check_against_composition(a, b, specs, wrap)


def _status(fn):
    with pytest.raises(N.CraftError) as e:
        fn()
    return e.value.status, str(e.value)


def test_stream_argument_errors_cpu():
    n = 8
    pool, specs = queue_inputs(W12, 12, n)
    sim = cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    out = stream_buffers(sim)
    acts = torch.zeros(n, dtype=torch.int32)
    # nothing installed yet
    assert _status(lambda: sim.begin_episodes())[0] == N.EINVAL
    assert _status(lambda: sim.step_stream(acts, **out))[0] == N.EINVAL
    sim.set_episode_queue(torch.as_tensor(specs))
    assert _status(lambda: sim.step_stream(acts, **out))[0] == N.EINVAL          # before begin
    # an invalid entry, one per field, at index 5: EINVAL naming it, and the old queue survives
    n_tasks = sim.config.n_tasks
    for col, bad in ((0, len(pool)), (0, -1), (1, 0), (1, 11), (2, 0), (2, 11), (3, 4), (3, -1), (4, n_tasks), (4, -1)):
        q = specs.copy()
        q[5, col] = bad
        q[9, col] = bad
        st, msg = _status(lambda: sim.set_episode_queue(torch.as_tensor(q)))
        assert st == N.EINVAL and "entry 5 " in msg, (col, bad, msg)
    for first, stride in ((len(specs) - n + 1, n), (len(specs), n), (-1, n), (0, 0), (0, -3)):
        assert _status(lambda: sim.begin_episodes(first=first, stride=stride))[0] == N.EINVAL
    sim.begin_episodes(first=len(specs), wrap=True)                             # fine under WRAP
    sim.begin_episodes(first=len(specs) - n)                                    # the last n entries
    now = torch.empty(n, dtype=torch.int32)
    sim.step_stream(acts, episode_now=now)                                      # the old queue is in force
    assert now.tolist() == list(range(len(specs) - n, len(specs)))
    st = sim.get_state()
    np.testing.assert_array_equal(st["spec"].numpy(), specs[len(specs) - n:])
    # flags other than AUTORESET
    args = N.craft_stream_step_args_t()
    args.step.actions = acts.data_ptr()
    for flags in (0, 2, 3):
        args.step.flags = flags
        assert sim._L.craft_step_stream(sim._h, ctypes.byref(args), None) == N.EINVAL
    # a bad action latches
    sim.step_stream(torch.full((n,), 6, dtype=torch.int32))
    with pytest.raises(N.CraftError) as e:
        sim.check()
    assert e.value.status == N.EBADACTION
    # a new queue needs a new begin
    sim.set_episode_queue(torch.as_tensor(specs[:n + 3]))
    assert _status(lambda: sim.step_stream(acts, **out))[0] == N.EINVAL
    sim.begin_episodes()
    sim.step_stream(acts, **out)
    sim.check()


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
def test_stream_sharding_cpu(wrap):
    """Two handles of n/2 with env_id_base 0 and n/2 and stride n, concatenated, equal one
    handle of n, for hashed-draw actions."""
    n, h = 40, 20
    pool, specs = queue_inputs(W12, 12, n)
    whole = cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    parts = [cpu_sim(W12, h, pool, max_timesteps=T_MAX, env_id_base=b) for b in (0, h)]
    for s in [whole] + parts:
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes(stride=n, wrap=wrap)
    restarts = 0
    for t in range(26):
        ow = stream_buffers(whole)
        whole.step_stream(None, seed=21, tick=t, **ow)
        op = [stream_buffers(s) for s in parts]
        for s, o in zip(parts, op):
            s.step_stream(None, seed=21, tick=t, **o)
        for k in ow:
            if k == "any_live":
                assert int(ow[k][0]) == max(int(o[k][0]) for o in op), t
            else:
                assert torch.equal(ow[k], torch.cat([o[k] for o in op])), (k, t)
        restarts += int((ow["episode_end"] >= 0).sum())
    assert restarts > n
    sw = whole.get_state()
    sp = [s.get_state() for s in parts]
    for k in sw:
        assert torch.equal(sw[k], torch.cat([x[k] for x in sp])), k
    assert torch.equal(whole.stats(), parts[0].stats() + parts[1].stats())


def test_evaluate_equals_do_rollout_cpu(golden):
    check_evaluate_equals_do_rollout(golden, "cpu")


def test_evaluate_equals_reference_cpu(golden):
    check_evaluate_equals_reference(golden, "cpu")
