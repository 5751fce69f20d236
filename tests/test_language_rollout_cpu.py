"""craft_step_lang (the language trainers' tick) and do_language_rollout through the CPU variant
of the C ABI: the reference's three language trainers' do_rollout (tests/golden/
language_rollout.npz), a per-env loop over the oracle, the argument errors.
tests/test_gpu_step_lang.py checks the HIP kernel against this."""
import ctypes

import numpy as np
import pytest
import torch

from psketch_amd import _native as N
from psketch_amd import sample_scenarios, synthetic_specs
from tests.helpers import make_tables
from tests.language_rollout_cases import (CASES, CASE_IDS, check_case, check_teacher_raise_of_ended_slot,
                                          make_sim)
from tests.test_cpu_variant import cpu_sim


@pytest.fixture(scope="module")
def fx(golden):
    return golden("language_rollout.npz")


@pytest.mark.parametrize("mode,is_eval,T", CASES, ids=CASE_IDS)
def test_language_rollout_cpu_vs_reference(fx, mode, is_eval, T):
    check_case(fx, make_sim(fx, T, "cpu"), mode, is_eval, T)


def lang_buffers(sim, dev="cpu"):
    n = sim.n_envs
    return dict(obs=torch.zeros((n, sim.n_features), dtype=sim.obs_dtype, device=dev),
                done=torch.full((n,), 9, dtype=torch.uint8, device=dev),
                success=torch.full((n,), 9, dtype=torch.int8, device=dev),
                action_record=torch.full((n,), 9, dtype=torch.int32, device=dev),
                ask_record=torch.full((n,), 9, dtype=torch.int8, device=dev),
                transition_code=torch.full((n,), 9, dtype=torch.int8, device=dev),
                any_live=torch.zeros(1, dtype=torch.int32, device=dev),
                labels=torch.full((n,), 9, dtype=torch.int32, device=dev))


def test_step_lang_cpu_vs_oracle(oracle_mod):
    """100 envs, 44 ticks at max_timesteps 40 (the last ticks run on all-frozen envs), random
    actions with a random use_alt mask, against the protocol written out over the oracle."""
    world, T = "craft_medium_12x12", 40
    params, cb, tm, cfg = make_tables(world, T)
    pool, _, _ = sample_scenarios(params, cb, 123, 32)
    n, ticks = 100, 44
    specs = synthetic_specs(pool, 12, 12, n, 0, seed=6, task_ids=[t.id for t in tm.dataset_tasks()])
    sim = cpu_sim(world, n, pool, max_timesteps=T)
    sim.reset(*specs)
    o = oracle_mod.Oracle(cfg, pool)
    envs = o.init_envs(*specs)
    timer = np.full(n, T)
    frozen = np.zeros(n, bool)
    rng = np.random.RandomState(12)
    stats = np.zeros(3, dtype=np.int64)
    ended_on_stop = ended_on_timer_nonidle = 0
    for t in range(ticks):
        acts = rng.choice(6, size=n, p=[.22, .22, .22, .22, .1, .02]).astype(np.int32)
        alt = rng.randint(0, 6, size=n).astype(np.int32)
        use = (rng.rand(n) < 0.4).astype(np.uint8)
        out = lang_buffers(sim)
        sim.step_lang(torch.as_tensor(acts), tick=t, alt_actions=torch.as_tensor(alt),
                      use_alt=torch.as_tensor(use), **out)
        exp = {k: np.zeros(n, dtype=np.int64) for k in
               ("done", "success", "action_record", "ask_record", "transition_code", "labels")}
        exp_obs = np.zeros((n, sim.n_features), dtype=np.float32)
        live = 0
        for i in range(n):
            e = envs[i:i + 1]
            was = frozen[i]
            rec = ask = code = -1
            if not was:
                a = int(alt[i]) if use[i] else int(acts[i])
                px, py, pinv = int(e["x"][0]), int(e["y"][0]), e["inv"][0].copy()
                assert o.step(e, a) == 0
                dx, dy = int(e["x"][0]) - px, int(e["y"][0]) - py
                if (dx, dy) == (0, 0):
                    code = 4 if (e["inv"][0] != pinv).any() else 5
                else:
                    code = {(0, -1): 0, (0, 1): 1, (-1, 0): 2, (1, 0): 3}[(dx, dy)]
                rec, ask = a, int(use[i])
                timer[i] -= 1
                stats[2] += 1
                if a == 5 or timer[i] <= 0:
                    frozen[i] = True
                    stats[1] += 1
                    stats[0] += o.satisfies(e, int(specs[4][i])) == 1
                    ended_on_stop += a == 5
                    ended_on_timer_nonidle += a != 5 and code != 5
                else:
                    live = 1
            exp["done"][i] = frozen[i]
            exp["success"][i] = o.satisfies(e, int(specs[4][i])) if frozen[i] else -1
            exp["action_record"][i], exp["ask_record"][i], exp["transition_code"][i] = rec, ask, code
            exp_obs[i] = o.features(e)
            if was:
                exp["labels"][i] = -1
            else:
                rc, lab = o.teacher(e, int(specs[4][i]))
                exp["labels"][i] = -2 if rc else lab
        for k, v in exp.items():
            got = out[k].numpy().astype(np.int64)
            if k == "labels":                    # compared for the slots still running
                run = ~frozen
                np.testing.assert_array_equal(got[run], v[run], err_msg=f"{k} tick {t}")
                assert (got[exp["action_record"] < 0] == -1).all()
            else:
                np.testing.assert_array_equal(got, v, err_msg=f"{k} tick {t}")
        np.testing.assert_array_equal(out["obs"].numpy(), exp_obs, err_msg=f"obs tick {t}")
        assert int(out["any_live"][0]) == live, f"any_live tick {t}"
    assert frozen.all() and ended_on_stop > 0 and ended_on_timer_nonidle > 0
    np.testing.assert_array_equal(sim.stats().numpy(), stats)
    # labels of the slots that ended are the teacher's too, or -2 where it raises (never
    # latched for them): the run latched nothing
    sim.check()


def test_step_lang_frozen_slots_behave_as_craft_step_froze_them():
    world = "craft_medium_12x12"
    params, cb, tm, cfg = make_tables(world, 3)
    pool, _, _ = sample_scenarios(params, cb, 123, 8)
    n = 20
    specs = synthetic_specs(pool, 12, 12, n, 0, seed=2, task_ids=[t.id for t in tm.dataset_tasks()])
    sim = cpu_sim(world, n, pool, max_timesteps=3)
    sim.reset(*specs)
    acts = torch.zeros(n, dtype=torch.int32)
    acts[::2] = N.STOP
    done = torch.zeros(n, dtype=torch.uint8)
    sim.step_lang(acts, done=done)
    assert done.tolist() == [1, 0] * (n // 2)
    before = sim.get_state()
    d2 = torch.zeros(n, dtype=torch.uint8)
    rec = torch.zeros(n, dtype=torch.int32)
    sim.step(torch.ones(n, dtype=torch.int32), autoreset=False, done=d2, action_record=rec)
    assert (d2[::2] == 1).all() and (rec[::2] == -1).all() and (rec[1::2] == 1).all()
    after = sim.get_state()
    np.testing.assert_array_equal(after["agent"][::2].numpy(), before["agent"][::2].numpy())
    assert (sim.teacher()[0][::2] == -1).all()
    sim.reset(*specs)
    sim.step_lang(acts, done=done, action_record=rec)
    assert (rec == acts).all()
    sim.check()


def test_step_lang_argument_errors():
    world = "craft_medium_12x12"
    params, cb, tm, cfg = make_tables(world)
    pool, _, _ = sample_scenarios(params, cb, 123, 4)
    n = 8
    specs = synthetic_specs(pool, 12, 12, n, 0, seed=2, task_ids=[t.id for t in tm.dataset_tasks()])
    sim = cpu_sim(world, n, pool)
    sim.reset(*specs)
    with pytest.raises(N.CraftError) as e:
        sim.step_lang(flags=N.STEP_AUTORESET)
    assert e.value.status == N.EINVAL
    with pytest.raises(N.CraftError) as e:
        sim.step_lang(use_alt=torch.ones(n, dtype=torch.uint8))
    assert e.value.status == N.EINVAL
    assert sim._L.craft_step_lang(sim._h, None, None) == N.EINVAL
    assert sim._L.craft_step_lang(None, ctypes.byref(N.craft_lang_step_args_t()), None) == N.EINVAL
    sim.check()                                   # none of them latched or stepped anything
    assert sim.stats().tolist() == [0, 0, 0]
    # an action outside 0..5 latches CRAFT_EBADACTION; the slot takes no step
    acts = torch.zeros(n, dtype=torch.int32)
    acts[3] = 6
    before = sim.get_state()
    rec = torch.zeros(n, dtype=torch.int32)
    code = torch.zeros(n, dtype=torch.int8)
    sim.step_lang(acts, action_record=rec, transition_code=code)
    with pytest.raises(N.CraftError) as e:
        sim.check()
    assert e.value.status == N.EBADACTION
    after = sim.get_state()
    np.testing.assert_array_equal(after["agent"][3].numpy(), before["agent"][3].numpy())
    assert rec[3] == -1 and code[3] == -1 and sim.stats().tolist()[2] == n - 1
    # the same through use_alt
    alt = torch.full((n,), -1, dtype=torch.int32)
    use = torch.zeros(n, dtype=torch.uint8)
    use[5] = 1
    sim.step_lang(torch.zeros(n, dtype=torch.int32), alt_actions=alt, use_alt=use)
    with pytest.raises(N.CraftError) as e:
        sim.check()
    assert e.value.status == N.EBADACTION


def test_fixture_holds_the_array_visible_conditions(fx):
    """An env whose episode the timer ends with a last step that did something, and one that
    ends on STOP: the two places the language tick differs from the imitation tick."""
    A = fx["interactive_train_12_action_seqs"]
    last = A[:, -1]
    assert ((A == N.STOP).any(axis=1)).any()
    # replay on the CPU variant to see the last transition code of the timer-ended envs
    sim = make_sim(fx, 12, "cpu")
    sim.reset(*fx["spec"].T.copy())
    code = torch.zeros(sim.n_envs, dtype=torch.int8)
    for t in range(12):
        sim.step_lang(torch.as_tensor(np.where(A[:, t] >= 0, A[:, t], 0).astype(np.int32)),
                      transition_code=code)
    sim.check()
    timer_ended = (last >= 0) & (last != N.STOP)
    assert timer_ended.any() and ((code.numpy() >= 0) & (code.numpy() != 5) & timer_ended).any()


def test_step_lang_teacher_raise_latches_only_for_running_slots():
    check_teacher_raise_of_ended_slot("cpu")
