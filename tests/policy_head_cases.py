"""Shared by tests/test_policy_head_cpu.py and tests/test_gpu_policy_head.py: the policy head
(include/craft.h "The head rule": craft_policy_actions, craft_step_policy, craft_step_policy_stream).
The logit rows of the head's own tests, the head's definition recomputed in Python integers and
float64, the closed loop whose logits are exact on every device, and the comparison of the fused
tick against the head followed by the wrapped entry point.  Every function takes the simulators it
compares, so one of them may be the HIP library and the other the CPU variant."""
import numpy as np
import torch

from psketch_amd import _native as N
from psketch_amd import sample_scenarios, synthetic_specs
from psketch_amd.rollout import do_rollout
from tests.helpers import make_tables
from tests.stream_cases import T_MAX, Coverage, host_outputs, stream_buffers

MODES = ("argmax", "sample")
HEAD_SEED = 0x5EEDFACE12345
NEG_INF = float("-inf")
EPS = 1e-5            # the issue's bound: six weights at 2^-21 relative, six adds, one multiply < 4e-6
M64 = (1 << 64) - 1


# ---- rows ---------------------------------------------------------------------------------------
def logit_rows(n, seed=4, dominated=False):
    """float32 [n, 6]: random normals x 3; rows with 2- to 6-way ties of the maximum; rows with 1
    to 5 entries at -inf; (dominated) rows like [0, -100, ...] and rows spread past the -80 clamp."""
    rng = np.random.RandomState(seed)
    L = (rng.standard_normal((n, 6)) * 3).astype(np.float32)
    kind = rng.randint(0, 4 if dominated else 3, size=n)
    for i in np.nonzero(kind == 1)[0]:                    # ties of the maximum
        k = rng.randint(2, 7)
        at = rng.choice(6, size=k, replace=False)
        L[i, at] = L[i].max() + np.float32(0.5)
    for i in np.nonzero(kind == 2)[0]:                    # masked actions
        k = rng.randint(1, 6)
        L[i, rng.choice(6, size=k, replace=False)] = NEG_INF
    for i in np.nonzero(kind == 3)[0]:                    # dominated rows
        L[i] = rng.choice([-100.0, -79.5, -80.5, -30.0, -3e38], size=6).astype(np.float32)
        L[i, rng.randint(0, 6)] = np.float32(rng.choice([0.0, 50.0, 3e38]))
    return L


def bad_rows():
    """Rows that yield -1: a NaN, a +inf (alone or beside a NaN or -inf), nothing but -inf."""
    nan, inf = float("nan"), float("inf")
    return np.asarray([[0, 1, nan, 2, 3, 4], [nan] * 6, [0, inf, 1, 2, 3, 4], [inf] * 6,
                       [NEG_INF] * 6, [NEG_INF, inf, 0, 0, 0, 0], [5, 4, 3, 2, 1, nan],
                       [nan, NEG_INF, NEG_INF, NEG_INF, NEG_INF, NEG_INF]], dtype=np.float32)


def on(sim, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=sim.device)


# ---- the definition, independent of both libraries -----------------------------------------------
def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def head_u(seed, gid, tick):
    """u of the head rule, exactly, from Python integers."""
    return (splitmix64((seed ^ (gid << 20) ^ tick) & M64) >> 40) / float(1 << 24)


def check_sample_against_definition(L, actions, seed, gid0, tick):
    """Every slot's action k satisfies CDF[k-1] - EPS <= u <= CDF[k] + EPS of the float64 softmax,
    and no masked action is drawn.  No slot is excused."""
    L64 = L.astype(np.float64)
    m = L64.max(1, keepdims=True)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isneginf(L64), 0.0, np.exp(np.maximum(L64 - m, -80.0)))
    cdf = np.cumsum(w, 1) / w.sum(1, keepdims=True)
    n = len(L)
    u = np.asarray([head_u(seed, gid0 + i, tick) for i in range(n)])
    k = actions.astype(np.int64)
    assert ((k >= 0) & (k < 6)).all()
    rows = np.arange(n)
    lo = np.where(k > 0, cdf[rows, np.maximum(k - 1, 0)], 0.0)
    hi = cdf[rows, k]
    bad = np.nonzero(~((lo - EPS <= u) & (u <= hi + EPS)))[0]
    assert len(bad) == 0, (bad[:5], u[bad[:5]], lo[bad[:5]], hi[bad[:5]], L[bad[:5]])
    assert not np.isneginf(L[rows, k]).any(), "a masked action was drawn"
    return u


def check_argmax(sim, n=4096):
    L = logit_rows(n)
    got = sim.policy_actions(on(sim, L), "argmax").cpu().numpy()
    np.testing.assert_array_equal(got, torch.argmax(torch.as_tensor(L), dim=1).numpy())
    ties = (L == L.max(1, keepdims=True)).sum(1)
    assert set(range(1, 7)) <= set(ties.tolist()) and np.isneginf(L).any()
    return got


def check_bad_rows(make_sim, modes=MODES):
    """Rows with a NaN or +inf, or all -inf, yield -1 under both modes; in step_policy such a row
    latches CRAFT_EBADACTION naming its slot, and check() is clean without one."""
    B = bad_rows()
    n = 24
    sim, specs = make_sim(n)
    L = logit_rows(n, seed=6)
    for mode in modes:
        for j, row in enumerate(B):
            slot = (5 * j + 3) % n
            Lb = L.copy()
            Lb[slot] = row
            got = sim.policy_actions(on(sim, Lb), mode, seed=HEAD_SEED, tick=j).cpu().numpy()
            assert got[slot] == -1 and (np.delete(got, slot) >= 0).all(), (mode, j, got)
            sim.reset(*specs)
            sim.step(logits=on(sim, L), head=mode, head_seed=HEAD_SEED, tick=j, autoreset=False)
            sim.check()                                   # clean without a bad row
            sim.reset(*specs)                             # (every slot running again)
            rec = torch.empty(n, dtype=torch.int32, device=sim.device)
            sim.step(logits=on(sim, Lb), head=mode, head_seed=HEAD_SEED, tick=j, autoreset=False,
                     action_record=rec)
            try:
                sim.check()
            except N.CraftError as e:
                assert e.status == N.EBADACTION and f"(slot/item {slot})" in str(e), (mode, j, str(e))
            else:
                raise AssertionError(f"row {j} did not latch ({mode})")
            assert int(rec[slot]) == -1


def sample_actions(sim, L, ticks=(0, 1, 2)):
    return np.stack([sim.policy_actions(on(sim, L), "sample", seed=HEAD_SEED, tick=t).cpu().numpy() for t in ticks])


def check_sharding(make_handle, n=512):
    """Two handles of n/2 with env_id_base 0 and n/2 draw the actions of one handle of n."""
    L = logit_rows(n, seed=9, dominated=True)
    whole = make_handle(n, 0)
    parts = [make_handle(n // 2, b) for b in (0, n // 2)]
    for t in (0, 3):
        w = whole.policy_actions(on(whole, L), "sample", seed=HEAD_SEED, tick=t).cpu().numpy()
        p = [s.policy_actions(on(s, L[b:b + n // 2]), "sample", seed=HEAD_SEED, tick=t).cpu().numpy()
             for s, b in zip(parts, (0, n // 2))]
        np.testing.assert_array_equal(w, np.concatenate(p))
        check_sample_against_definition(L, w, HEAD_SEED, 0, t)
    assert len(set(w.tolist())) == 6


# ---- the closed loop -------------------------------------------------------------------------------
def int_weights(F, seed=7):
    """A fixed seeded integer matrix in [-3, 3]: with the small-integer observations every sum
    of obs @ Wint is exact in fp32 in any order, so every device computes the same logits."""
    return np.random.RandomState(seed).randint(-3, 4, size=(F, 6)).astype(np.float32)


def closed_loop_logits(sim, W):
    Wd = on(sim, W)

    def logits(obs):
        return ((obs.to(torch.float32) @ Wd) * 0.25).contiguous()
    return logits


STEP_OUTPUTS = ("obs", "reward", "done", "success", "action_record", "transition_code", "labels")


def step_buffers(sim, teach):
    o = stream_buffers(sim, teach)
    return {k: o[k] for k in STEP_OUTPUTS + ("any_live",)}


def same_check(a, b):
    """check() of both: the same status (and slot) or both clean."""
    def one(s):
        try:
            s.check()
        except N.CraftError as e:
            return e.status, str(e)
        return 0, ""
    assert one(a) == one(b)


def compare_tick(oa, ob, t, names):
    for k in names:
        if oa[k] is None:
            assert ob[k] is None
            continue
        assert torch.equal(oa[k].cpu(), ob[k].cpu()), f"{k} at tick {t}"


def compare_handles(a, b, t):
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k].cpu(), sb[k].cpu()), (k, t)
    assert torch.equal(a.stats().cpu(), b.stats().cpu()), t
    same_check(a, b)


def world_inputs(world, W, n, H=None, seed=11, pool_size=24, max_timesteps=T_MAX, tables=None):
    params, cb, tm, cfg = tables or make_tables(world, max_timesteps)
    pool, _, _ = sample_scenarios(params, cb, 123, pool_size)
    specs = synthetic_specs(pool, W, W if H is None else H, n, 0, seed=seed,
                            task_ids=[t.id for t in tm.dataset_tasks()])
    return pool, [np.ascontiguousarray(s) for s in specs]


def run_fused_vs_split(a, b, specs, mode, teach, autoreset, ticks=12):
    """Handle a runs craft_step_policy; its twin b craft_policy_actions followed by craft_step_ex
    (teach False) or craft_step_teach.  Logits from each handle's own observations; behavior_clone
    on a third of the slots (their labels: the teacher's, or without a teacher in the launch a
    seeded draw).  After every tick every output buffer, get_state(), stats() and check()."""
    n = a.n_envs
    W = int_weights(a.n_features)
    la, lb = closed_loop_logits(a, W), closed_loop_logits(b, W)
    obs_a, obs_b = a.empty_obs(), b.empty_obs()
    a.reset(*specs, obs=obs_a)
    b.reset(*specs, obs=obs_b)
    bc = (np.arange(n) % 3 == 1).astype(np.uint8)
    rng = np.random.RandomState(2)
    ref_a, ref_b = (a.teacher()[0], b.teacher()[0]) if teach else (None, None)
    seen, ends = set(), 0
    for t in range(ticks):
        if not teach:
            r = rng.randint(0, 6, size=n).astype(np.int32)
            ref_a, ref_b = on(a, r), on(b, r)
        oa, ob = step_buffers(a, teach), step_buffers(b, teach)
        oa["obs"], ob["obs"] = obs_a, obs_b
        logits_a, logits_b = la(obs_a), lb(obs_b)
        assert torch.equal(logits_a.cpu(), logits_b.cpu()), t
        a.step(logits=logits_a, head=mode, head_seed=HEAD_SEED, tick=t, autoreset=autoreset,
               ref_actions=ref_a, behavior_clone=on(a, bc), **oa)
        acts = b.policy_actions(logits_b, mode, seed=HEAD_SEED, tick=t)
        b.step(acts, tick=t, autoreset=autoreset, ref_actions=ref_b, behavior_clone=on(b, bc), **ob)
        compare_tick(oa, ob, t, STEP_OUTPUTS + ("any_live",))
        compare_handles(a, b, t)
        rec = ob["action_record"].cpu().numpy()
        taken = np.where(bc == 1, -1, rec)
        np.testing.assert_array_equal(taken[(bc == 0) & (rec >= 0)], acts.cpu().numpy()[(bc == 0) & (rec >= 0)])
        seen |= set(taken[taken >= 0].tolist())
        ends += int((ob["done"].cpu().numpy() == 1).sum())
        if teach:
            ref_a, ref_b = oa["labels"].clone(), ob["labels"].clone()
    # the head chose among the actions (one env alone sees few of them); episodes ended
    assert len(seen) >= (4 if n >= 40 else 1) and ends > 0, (seen, ends)


def run_stream_fused_vs_split(a, b, specs, mode, wrap, teach=True, ticks=30):
    """The same for craft_step_policy_stream against craft_policy_actions + craft_step_stream, on
    stream_cases' queue; asserts from b's outputs that restarts, STOP endings and timeouts occurred."""
    n = a.n_envs
    W = int_weights(a.n_features)
    W[:, N.STOP] += np.float32(1.0) * (np.arange(a.n_features) % 5 == 0)      # STOP now and then
    la, lb = closed_loop_logits(a, W), closed_loop_logits(b, W)
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
    obs_a, obs_b = a.empty_obs(), b.empty_obs()
    a.begin_episodes(wrap=wrap, obs=obs_a)
    b.begin_episodes(wrap=wrap, obs=obs_b)
    bc = (np.arange(n) % 3 == 1).astype(np.uint8)
    ref_a, ref_b = a.teacher()[0], b.teacher()[0]
    cov = Coverage(specs, n, wrap)
    names = STEP_OUTPUTS + ("any_live", "episode_end", "end_pose", "episode_now")
    for t in range(ticks):
        oa, ob = stream_buffers(a, teach), stream_buffers(b, teach)
        oa["obs"], ob["obs"] = obs_a, obs_b
        logits_a, logits_b = la(obs_a), lb(obs_b)
        assert torch.equal(logits_a.cpu(), logits_b.cpu()), t
        a.step_stream(logits=logits_a, head=mode, head_seed=HEAD_SEED, tick=t, ref_actions=ref_a,
                      behavior_clone=on(a, bc), **oa)
        acts = b.policy_actions(logits_b, mode, seed=HEAD_SEED, tick=t)
        b.step_stream(acts, tick=t, ref_actions=ref_b, behavior_clone=on(b, bc), **ob)
        compare_tick(oa, ob, t, names)
        compare_handles(a, b, t)
        cov.tick(None, host_outputs(ob))
        if teach:
            ref_a, ref_b = oa["labels"].clone(), ob["labels"].clone()
        else:
            ref_a, ref_b = a.teacher()[0], b.teacher()[0]
    cov.check()


# ---- the drivers -----------------------------------------------------------------------------------
def rollout_fixture(golden, device, case="dev8"):
    """The reference fixture's inputs (tests/golden/imitation_rollout.npz, 32 envs): a simulator,
    its specs, the behaviour-cloning mask."""
    from psketch_amd import CraftSim
    fx = golden("imitation_rollout.npz")
    world = {"dev8": "craft_medium", "w12": "craft_medium_12x12"}[case]
    pool, spec = fx[f"{case}_pool"], fx[f"{case}_spec"]
    sim = CraftSim(world, n_envs=len(spec), device=device, pool_capacity=len(pool))
    sim.load_pool(pool)
    return sim, tuple(np.ascontiguousarray(c) for c in spec.T), fx[f"{case}_train_bc"]


def check_do_rollout_head(golden, device, is_eval, graph=0):
    """do_rollout(head="argmax") with act returning logits gives the RolloutInfo of do_rollout
    with act returning argmax of those logits."""
    sim, spec, bc = rollout_fixture(golden, device)
    logits = closed_loop_logits(sim, int_weights(sim.n_features, seed=3))
    received = [[], []]

    def act_logits(obs, t):
        return logits(obs)

    def act_argmax(obs, t):
        return logits(obs).argmax(dim=1).to(torch.int32)

    kw = dict(behavior_clone=bc, graph=graph)
    a = do_rollout(sim, spec, act_logits, is_eval, head="argmax", receive=lambda r: received[0].append(r.cpu().numpy().copy()), **kw)
    b = do_rollout(sim, spec, act_argmax, is_eval, receive=lambda r: received[1].append(r.cpu().numpy().copy()), **kw)
    assert a.to_reference() == b.to_reference()
    assert a.ticks == b.ticks and torch.equal(a.action_seqs.cpu(), b.action_seqs.cpu())
    assert torch.equal(a.success.cpu(), b.success.cpu()) and torch.equal(a.distances.cpu(), b.distances.cpu())
    assert len(received[0]) == len(received[1]) == (0 if is_eval else a.ticks)
    for x, y in zip(*received):
        np.testing.assert_array_equal(x, y)
    assert len(set(a.action_seqs.cpu().numpy().ravel().tolist()) - {-1}) >= 3


def check_evaluate_head(golden, device, count=64):
    """evaluate(head="argmax") equals evaluate with the argmax act, on 64 dev instances."""
    from tests.evaluate_cases import N_ENVS, dev_instances, runner_for
    ds, items = dev_instances(golden)
    items = items[:count]
    runner = runner_for(ds, device)
    sim = runner.sim(N_ENVS)
    logits = closed_loop_logits(sim, int_weights(sim.n_features, seed=3))
    a = runner.evaluate(items, lambda obs, ctx: logits(obs), n_envs=N_ENVS, head="argmax")
    b = runner.evaluate(items, lambda obs, ctx: logits(obs).argmax(dim=1).to(torch.int32), n_envs=N_ENVS)
    assert a.eval_info == b.eval_info and len(a.eval_info) == count
    assert a.success_rate == b.success_rate and a.avg_distance == b.avg_distance and a.ticks == b.ticks
