"""Shared by tests/test_stream_cpu.py and tests/test_gpu_step_stream.py: the episode queue's
inputs, the lockstep comparison of two simulators running craft_step_stream, and the tick
against the composition of the entry points it fuses (craft_step without auto-reset, then
craft_set_state of the ended slots to their next queue entry, craft_observe, craft_teacher)."""
import numpy as np
import torch

from psketch_amd import _native as N
from psketch_amd import sample_scenarios, synthetic_specs
from tests.helpers import make_tables

T_MAX = 6            # max_timesteps of the stream tests
TICKS = 30
STREAM_OUTPUTS = ("obs", "reward", "done", "success", "action_record", "transition_code", "labels",
                  "episode_end", "end_pose", "episode_now")


def queue_inputs(world, W, n, seed=11, pool_size=24, H=None, tables=None):
    """A pool of `pool_size` scenarios and a queue of 3n + 17 episode specs over it (not a
    multiple of n: slots run out on different ticks), in shuffled order so that a slot's
    consecutive entries differ in scenario and task whatever n is, with every start direction.
    tables: make_tables' result for a cookbook and task list other than the built-in ones."""
    params, cb, tm, cfg = tables or make_tables(world, T_MAX)
    pool, _, _ = sample_scenarios(params, cb, 123, pool_size)
    count = 3 * n + 17
    specs = np.stack(synthetic_specs(pool, W, W if H is None else H, count, 0, seed=seed,
                                     task_ids=[t.id for t in tm.dataset_tasks()]), 1).astype(np.int32)
    rng = np.random.RandomState(seed)
    specs = specs[rng.permutation(count)]
    specs[:, 3] = rng.randint(0, 4, size=count)
    return pool, np.ascontiguousarray(specs)


def stream_buffers(sim, teach=True):
    n, dev = sim.n_envs, sim.device
    out = {"obs": sim.empty_obs(),
           "reward": torch.empty(n, dtype=torch.float32, device=dev),
           "done": torch.empty(n, dtype=torch.uint8, device=dev),
           "success": torch.empty(n, dtype=torch.int8, device=dev),
           "action_record": torch.empty(n, dtype=torch.int32, device=dev),
           "transition_code": torch.empty(n, dtype=torch.int8, device=dev),
           "any_live": torch.zeros(1, dtype=torch.int32, device=dev),
           "labels": torch.empty(n, dtype=torch.int32, device=dev) if teach else None,
           "episode_end": torch.empty(n, dtype=torch.int32, device=dev),
           "end_pose": torch.empty(n, dtype=torch.int32, device=dev),
           "episode_now": torch.empty(n, dtype=torch.int32, device=dev)}
    return out


def draw_actions(rng, n):
    """A seeded draw with STOP at about 10 %."""
    return rng.choice(6, size=n, p=[.18, .18, .18, .18, .18, .10]).astype(np.int32)


class Coverage:
    """What a stream run has exercised, from one simulator's outputs: the tests assert all of it
    so that they cannot pass vacuously."""

    def __init__(self, specs, n, wrap):
        self.specs, self.wrap = specs, wrap
        self.timer = np.full(n, T_MAX)
        self.new_scenario = self.new_task = self.ran_out = self.timeout = self.stop = 0

    def tick(self, acts, out):
        end, now = out["episode_end"], out["episode_now"]
        rec = out["action_record"]
        ended = end >= 0
        self.timer[rec >= 0] -= 1
        self.stop += int((ended & (rec == N.STOP)).sum())
        self.timeout += int((ended & (rec != N.STOP) & (self.timer <= 0)).sum())
        moved = ended & (now >= 0)
        self.new_scenario += int((self.specs[end[moved], 0] != self.specs[now[moved], 0]).sum())
        self.new_task += int((self.specs[end[moved], 4] != self.specs[now[moved], 4]).sum())
        self.ran_out += int((ended & (now < 0)).sum())
        self.timer[ended] = T_MAX

    def check(self):
        assert self.new_scenario > 0 and self.new_task > 0, "no restart onto a new scenario / task"
        assert self.timeout > 0 and self.stop > 0, "no episode ended by timeout / by STOP"
        if not self.wrap:
            assert self.ran_out > 0, "no slot ran out"


def host_outputs(out):
    """The outputs as numpy arrays (obs apart: bf16 has no numpy type)."""
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None and k != "obs"}


def run_lockstep(a, b, specs, wrap, teach=True, hashed_every=5):
    """Simulators a and b (the same world, pool and n) through the same stream of TICKS ticks:
    every output of every tick, then get_state() and stats(), must be equal.  Without wrap the
    run must see any_live stay 0 for two ticks."""
    n = a.n_envs
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
    oa0, ob0 = a.empty_obs(), b.empty_obs()
    a.begin_episodes(wrap=wrap, obs=oa0)
    b.begin_episodes(wrap=wrap, obs=ob0)
    assert torch.equal(oa0.cpu(), ob0.cpu())
    cov = Coverage(specs, n, wrap)
    rng = np.random.RandomState(3)
    idle = 0
    for t in range(TICKS):
        acts = draw_actions(rng, n)
        oa, ob = stream_buffers(a, teach), stream_buffers(b, teach)
        if hashed_every and t % hashed_every == hashed_every - 1:      # the hashed draw
            a.step_stream(None, seed=9, tick=t, **oa)
            b.step_stream(None, seed=9, tick=t, **ob)
        else:
            a.step_stream(torch.as_tensor(acts, device=a.device), tick=t, **oa)
            b.step_stream(torch.as_tensor(acts, device=b.device), tick=t, **ob)
        ha, hb = host_outputs(oa), host_outputs(ob)
        for k in ha:
            np.testing.assert_array_equal(ha[k], hb[k], err_msg=f"{k} at tick {t}")
        assert torch.equal(oa["obs"].cpu(), ob["obs"].cpu()), f"obs at tick {t}"
        cov.tick(acts, hb)
        idle = idle + 1 if int(hb["any_live"][0]) == 0 else 0
    if not wrap:
        assert idle >= 2, "the pass did not end"
        assert (hb["episode_now"] == -1).all() and (hb["done"] == 1).all()
    else:
        assert idle == 0
    cov.check()
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k].cpu(), sb[k].cpu()), k
    np.testing.assert_array_equal(a.stats().cpu().numpy(), b.stats().cpu().numpy())
    a.check()
    b.check()


def check_against_composition(a, b, specs, wrap):
    """Sim a runs craft_step_stream; sim b the pieces it fuses: craft_step without auto-reset with
    the same actions, then for the slots that ended this tick craft_set_state to their next queue
    entry (timer = max_timesteps, empty inventory), then craft_observe and craft_teacher.  Every
    output, get_state() (spec included) and stats() must be equal every tick."""
    n, dev, count = a.n_envs, a.device, len(specs)
    a.set_episode_queue(torch.as_tensor(specs))
    oa0, ob0 = a.empty_obs(), b.empty_obs()
    a.begin_episodes(wrap=wrap, obs=oa0)
    b.reset(*[specs[:n, j] for j in range(5)], obs=ob0)
    assert torch.equal(oa0, ob0)
    cur = np.arange(n)
    frozen = np.zeros(n, bool)
    cov = Coverage(specs, n, wrap)
    rng = np.random.RandomState(5)
    idle = 0
    K = a.n_kinds
    for t in range(TICKS):
        acts = draw_actions(rng, n)
        oa, ob = stream_buffers(a), stream_buffers(b)
        a.step_stream(torch.as_tensor(acts, device=dev), tick=t, **oa)
        b.step(torch.as_tensor(acts, device=dev), tick=t, autoreset=False,
               **{k: ob[k] for k in ("obs", "reward", "done", "success", "action_record", "transition_code")})
        hb = host_outputs(ob)
        ended = (hb["done"] == 1) & ~frozen
        agent = b.get_state(fields=("agent",))["agent"].cpu().numpy()
        exp_end = np.where(ended, cur, -1)
        exp_pose = np.where(ended, agent[:, 0] | (agent[:, 1] << 8) | (agent[:, 2] << 16), -1)
        nxt = cur + n
        nxt = nxt % count if wrap else np.where(nxt < count, nxt, -1)
        cur = np.where(ended, nxt, cur)
        frozen = frozen | (ended & (cur < 0))
        go = np.nonzero(ended & (cur >= 0))[0]
        if len(go):
            e = specs[cur[go]]
            b.set_state(torch.as_tensor(e), torch.as_tensor(np.concatenate([e[:, 1:4], np.full((len(go), 1), T_MAX)], 1)),
                        torch.zeros((len(go), K), dtype=torch.int32), slots=torch.as_tensor(go.astype(np.int32)))
        b.observe(obs=ob["obs"])
        labels, _ = b.teacher()
        ha = host_outputs(oa)
        for k in ("reward", "done", "success", "action_record", "transition_code"):
            np.testing.assert_array_equal(ha[k], hb[k], err_msg=f"{k} at tick {t}")
        assert torch.equal(oa["obs"], ob["obs"]), t
        np.testing.assert_array_equal(ha["labels"], labels.cpu().numpy(), err_msg=f"labels at tick {t}")
        assert (ha["labels"][frozen] == -1).all()
        np.testing.assert_array_equal(ha["episode_end"], exp_end, err_msg=f"episode_end at tick {t}")
        np.testing.assert_array_equal(ha["end_pose"], exp_pose, err_msg=f"end_pose at tick {t}")
        np.testing.assert_array_equal(ha["episode_now"], np.where(frozen, -1, cur), err_msg=f"episode_now at tick {t}")
        assert int(ha["any_live"][0]) == int((~frozen).any()), t
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (k, t)
        cov.tick(acts, ha)
        idle = idle + 1 if not (~frozen).any() else 0
    if not wrap:
        assert idle >= 2, "the pass did not end"
    cov.check()
    np.testing.assert_array_equal(a.stats().cpu().numpy(), b.stats().cpu().numpy())
    a.check()
    b.check()
