"""rollout.evaluate (one pass over a split on the episode queue), shared by the CPU and GPU test
files: against do_rollout(is_eval=True) on batches of 32, which the reference's fixture pins
(tests/golden/imitation_rollout.npz), and against tests/golden/imitation_evaluate.npz, the
reference's own ImitationTrainer.evaluate (tests/golden/make_golden_evaluate.py)."""
import numpy as np
import torch

from psketch_amd.dataset import Dataset
from psketch_amd.rollout import ImitationRollout
from tests.helpers import make_tables
from tests.test_host import devtest_as_json

N_INSTANCES, N_ENVS, T_MAX = 150, 32, 12


def dev_instances(golden):
    """The first 150 instances of the committed dev split, in dataset order, and its pool."""
    fx = golden("devtest.npz")
    _, cb, tm, _ = make_tables("craft_medium")
    ds = Dataset(devtest_as_json(fx, "dev", tm, cb.n_kinds), "dev", tm, random=np.random.RandomState(1),
                 batch_size=N_ENVS)
    return ds, ds.data[:N_INSTANCES]


def runner_for(ds, device):
    return ImitationRollout("craft_medium", ds.pool_array(), device=device, max_timesteps=T_MAX)


def check_evaluate_equals_do_rollout(golden, device):
    """A stateless policy that is exact in integers (CPU and GPU agree): per instance id the
    same actions and success as do_rollout(is_eval=True) on batches of 32, and the same success
    rate and mean distance."""
    ds, items = dev_instances(golden)
    runner = runner_for(ds, device)
    F = runner.sim(N_ENVS).n_features
    dev = runner.sim(N_ENVS).device
    w = torch.as_tensor(np.random.RandomState(2).randint(1, 1000, size=F), dtype=torch.int64, device=dev)

    def act(obs, _):
        return ((obs.to(torch.int64) * w).sum(1) % 6).to(torch.int32)

    expect, succ, dist = {}, [], []
    for lo in range(0, len(items), N_ENVS):
        batch = items[lo:lo + N_ENVS]
        ref = runner.do_rollout(batch, act, is_eval=True).to_reference()
        for it, seq, s in zip(batch, ref["action_seqs"], ref["success"]):
            expect[it["id"]] = {"actions": seq, "success": int(s)}
        succ += ref["success"]
        dist += ref["distances"]
    info = runner.evaluate(items, act, n_envs=N_ENVS)
    assert info.eval_info == expect
    assert info.success_rate == sum(succ) / len(succ) * 100
    assert info.avg_distance == sum(dist) / len(dist)
    # the policy ends episodes both ways, fails some get tasks away from their target, and the
    # pass is shorter than the batches' (no slot waits for the slowest of its batch)
    n_act = np.asarray([len(v["actions"]) for v in expect.values()])
    assert (n_act == T_MAX).any() and (n_act < T_MAX).any() and 0 < sum(succ) < len(succ) and sum(dist) > 0
    assert info.ticks <= sum(max(len(expect[it["id"]]["actions"]) for it in items[lo:lo + N_ENVS])
                             for lo in range(0, len(items), N_ENVS))


def check_evaluate_equals_reference(golden, device):
    """The fixture's table replayed through evaluate via ctx.episode / ctx.tick: per instance
    the reference's actions and success, its success rate and its mean distance."""
    fx = golden("imitation_evaluate.npz")
    assert int(fx["max_timesteps"]) == T_MAX and len(fx["ids"]) == N_INSTANCES
    ds, items = dev_instances(golden)
    # (the same instances in the same order: devtest.npz keeps the number of the reference's id)
    assert [it["id"].split("_")[1] for it in items] == [str(i).split("_")[1] for i in fx["ids"]]
    runner = runner_for(ds, device)
    sim = runner.sim(N_ENVS)
    table = torch.as_tensor(fx["table"].astype(np.int32), device=sim.device)
    seen_restart = []

    def act(obs, ctx):
        seen_restart.append(int(ctx.restarted.sum()))
        assert bool(((ctx.tick == 0) | (ctx.restarted == 0)).all())
        e = ctx.episode.clamp(min=0).long()
        return table[e, ctx.tick.clamp(max=T_MAX - 1).long()]

    info = runner.evaluate(items, act, n_envs=N_ENVS)
    assert seen_restart[0] == N_ENVS and sum(seen_restart) == N_INSTANCES
    for i, it in enumerate(items):
        a = fx["actions"][i]
        assert info.eval_info[it["id"]] == {"actions": [int(x) for x in a[a >= 0]], "success": int(fx["success"][i])}, it["id"]
    assert info.success_rate == float(fx["success_rate"])
    assert info.avg_distance == float(fx["avg_distance"])
