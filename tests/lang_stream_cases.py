"""Shared by tests/test_lang_stream_cpu.py and tests/test_gpu_step_lang_stream.py: the lockstep
comparison of two simulators running craft_step_lang_stream, the tick against the composition of
the entry points it fuses (craft_step_lang, then craft_set_state of the ended slots to their next
queue entry, craft_observe and craft_teacher), and the end-on-a-grab known-answer test: an
episode whose ending step changes inventory and mask in the very lane that then restarts.

Every third slot acts on alt_actions (use_alt, the active trainer's ASK bit), which are the
previous tick's teacher labels, so those slots follow the demonstration and some episodes end
with their task satisfied."""
import numpy as np
import torch

from psketch_amd import _native as N
from psketch_amd import sample_scenarios
from tests.helpers import make_tables
from tests.stream_cases import TICKS, Coverage, draw_actions, host_outputs

LANG_STREAM_OUTPUTS = ("obs", "done", "success", "action_record", "ask_record", "transition_code", "labels",
                       "episode_end", "end_pose", "episode_now")
LANG_OUTPUTS = ("obs", "done", "success", "action_record", "ask_record", "transition_code", "any_live", "labels")
GRABBED = 4          # transition code of a USE that took an item (include/craft.h)


def lang_stream_buffers(sim, teach=True):
    n, dev = sim.n_envs, sim.device
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)   # noqa: E731
    return {"obs": sim.empty_obs(),
            "done": torch.empty(n, dtype=torch.uint8, device=dev),
            "success": torch.empty(n, dtype=torch.int8, device=dev),
            "action_record": i32(),
            "ask_record": torch.empty(n, dtype=torch.int8, device=dev),
            "transition_code": torch.empty(n, dtype=torch.int8, device=dev),
            "any_live": torch.zeros(1, dtype=torch.int32, device=dev),
            "labels": i32() if teach else None,
            "episode_end": i32(), "end_pose": i32(), "episode_now": i32()}


def ask_mask(n):
    """Every third slot acts on alt_actions."""
    return (np.arange(n) % 3 == 0).astype(np.uint8)


def alt_from_labels(labels, acts):
    """The previous tick's labels as this tick's alt_actions; where there is none (-1: the slot was
    frozen, -2: the teacher raised) the drawn action, so that no slot is given a bad action."""
    return np.where((labels >= 0) & (labels < 6), labels, acts).astype(np.int32)


class LangCoverage(Coverage):
    """Coverage's counters, and the language protocol's own: an ending tick that grabbed, an
    episode that ended with its task satisfied."""

    def __init__(self, specs, n, wrap):
        super().__init__(specs, n, wrap)
        self.grab_end = self.success = 0

    def tick(self, acts, out):
        super().tick(acts, out)
        ended = out["episode_end"] >= 0
        self.grab_end += int((ended & (out["transition_code"] == GRABBED)).sum())
        self.success += int((ended & (out["success"] == 1)).sum())

    def check(self):
        super().check()
        assert self.grab_end >= 1, "no episode ended on a step that grabbed"
        assert self.success >= 1, "no episode ended with its task satisfied"


def _step(sim, acts, alt, ask, t, out, hashed):
    dev = sim.device
    sim.step_lang_stream(None if hashed else torch.as_tensor(acts, device=dev), seed=9, tick=t,
                         alt_actions=torch.as_tensor(alt, device=dev), use_alt=torch.as_tensor(ask, device=dev), **out)


def run_lang_lockstep(a, b, specs, wrap, teach=True, hashed_every=5):
    """Simulators a and b (the same world, pool and n) through the same stream of TICKS ticks of
    craft_step_lang_stream: every output of every tick, then get_state() and stats(), must be
    equal.  b always runs the teacher (its labels are the next tick's alt_actions); a only with
    `teach`.  Without wrap the run must see any_live stay 0 for two ticks."""
    n = a.n_envs
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
    oa0, ob0 = a.empty_obs(), b.empty_obs()
    a.begin_episodes(wrap=wrap, obs=oa0)
    b.begin_episodes(wrap=wrap, obs=ob0)
    assert torch.equal(oa0.cpu(), ob0.cpu())
    cov = LangCoverage(specs, n, wrap)
    rng = np.random.RandomState(3)
    ask = ask_mask(n)
    labels = b.teacher()[0].cpu().numpy()
    idle = 0
    for t in range(TICKS):
        acts = draw_actions(rng, n)
        alt = alt_from_labels(labels, acts)
        oa, ob = lang_stream_buffers(a, teach), lang_stream_buffers(b, True)
        hashed = bool(hashed_every) and t % hashed_every == hashed_every - 1
        _step(a, acts, alt, ask, t, oa, hashed)
        _step(b, acts, alt, ask, t, ob, hashed)
        ha, hb = host_outputs(oa), host_outputs(ob)
        for k in ha:
            np.testing.assert_array_equal(ha[k], hb[k], err_msg=f"{k} at tick {t}")
        assert torch.equal(oa["obs"].cpu(), ob["obs"].cpu()), f"obs at tick {t}"
        cov.tick(acts, hb)
        labels = hb["labels"]
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
    # (a teacher raise of a running slot latches in both or in neither)
    assert int(a.error_word().cpu()[0]) == int(b.error_word().cpu()[0])
    return cov


def check_lang_against_composition(a, b, specs, wrap, ticks=TICKS, check_cov=True):
    """Sim a runs craft_step_lang_stream; sim b the pieces it fuses: craft_step_lang with the same
    actions, then for the slots that ended this tick and have a next queue entry craft_set_state
    to it (timer = max_timesteps, empty inventory), then craft_observe and craft_teacher of those
    slots.  Every output, get_state() (spec included) and stats() must be equal every tick."""
    n, dev, count = a.n_envs, a.device, len(specs)
    T = a.config.max_timesteps
    a.set_episode_queue(torch.as_tensor(specs))
    oa0, ob0 = a.empty_obs(), b.empty_obs()
    a.begin_episodes(wrap=wrap, obs=oa0)
    b.reset(*[specs[:n, j] for j in range(5)], obs=ob0)
    assert torch.equal(oa0, ob0)
    cur = np.arange(n)
    frozen = np.zeros(n, bool)
    cov = LangCoverage(specs, n, wrap)
    rng = np.random.RandomState(5)
    ask = ask_mask(n)
    labels = b.teacher()[0].cpu().numpy()
    idle = 0
    K = a.n_kinds
    for t in range(ticks):
        acts = draw_actions(rng, n)
        alt = alt_from_labels(labels, acts)
        oa, ob = lang_stream_buffers(a), lang_stream_buffers(b)
        _step(a, acts, alt, ask, t, oa, False)
        b.step_lang(torch.as_tensor(acts, device=dev), tick=t, alt_actions=torch.as_tensor(alt, device=dev),
                    use_alt=torch.as_tensor(ask, device=dev), **{k: ob[k] for k in LANG_OUTPUTS})
        hb = host_outputs(ob)
        ended = (hb["done"] == 1) & ~frozen
        agent = b.get_state(fields=("agent",))["agent"].cpu().numpy()     # the post-step pose
        exp_end = np.where(ended, cur, -1)
        exp_pose = np.where(ended, agent[:, 0] | (agent[:, 1] << 8) | (agent[:, 2] << 16), -1)
        nxt = cur + n
        nxt = nxt % count if wrap else np.where(nxt < count, nxt, -1)
        cur = np.where(ended, nxt, cur)
        frozen = frozen | (ended & (cur < 0))
        go = np.nonzero(ended & (cur >= 0))[0]
        exp_labels = hb["labels"].copy()
        if len(go):
            e = specs[cur[go]]
            slots = torch.as_tensor(go.astype(np.int32), device=dev)
            b.set_state(torch.as_tensor(e), torch.as_tensor(np.concatenate([e[:, 1:4], np.full((len(go), 1), T)], 1)),
                        torch.zeros((len(go), K), dtype=torch.int32), slots=slots)
            rows = b.empty_obs(len(go))
            b.observe(slots=slots, obs=rows)
            ob["obs"][slots.long()] = rows
            exp_labels[go] = b.teacher(slots=slots)[0].cpu().numpy()
        ha = host_outputs(oa)
        for k in ("done", "success", "action_record", "ask_record", "transition_code"):
            np.testing.assert_array_equal(ha[k], hb[k], err_msg=f"{k} at tick {t}")
        assert torch.equal(oa["obs"], ob["obs"]), t
        np.testing.assert_array_equal(ha["labels"], exp_labels, err_msg=f"labels at tick {t}")
        np.testing.assert_array_equal(ha["episode_end"], exp_end, err_msg=f"episode_end at tick {t}")
        np.testing.assert_array_equal(ha["end_pose"], exp_pose, err_msg=f"end_pose at tick {t}")
        np.testing.assert_array_equal(ha["episode_now"], np.where(frozen, -1, cur), err_msg=f"episode_now at tick {t}")
        assert int(ha["any_live"][0]) == int((~frozen).any()), t
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (k, t)
        cov.tick(acts, ha)
        labels = ha["labels"]
        idle = idle + 1 if not (~frozen).any() else 0
    if not wrap:
        assert idle >= 2, "the pass did not end"
    if check_cov:
        cov.check()
    np.testing.assert_array_equal(a.stats().cpu().numpy(), b.stats().cpu().numpy())
    return cov


# ---- the end-on-a-grab known-answer test ------------------------------------------------------------

_DX, _DY = (0, 0, -1, 1), (-1, 1, 0, 0)      # DOWN, UP, LEFT, RIGHT (craft.py)


def grab_queue(world, W, H, n, pool_size=24):
    """A pool and 3n + 17 queue entries whose pose faces a cell holding its own get task's kind, found
    by scanning the pool: a USE on the first tick grabs it and satisfies the task."""
    params, cb, tm, cfg = make_tables(world, 1)
    pool, _, _ = sample_scenarios(params, cb, 123, pool_size)
    grids = np.asarray(pool).reshape(pool_size, W, H)
    gets = [(t, cfg.task[t].arg_kind) for t in range(cfg.n_tasks) if cfg.task[t].goal == N.GOAL_GET
            and cfg.kind_class[cfg.task[t].arg_kind] == N.KIND_GRABBABLE]
    found = []
    for sc in range(pool_size):
        for x in range(1, W - 1):
            for y in range(1, H - 1):
                if grids[sc, x, y] != 0:
                    continue
                for d in range(4):
                    k = grids[sc, x + _DX[d], y + _DY[d]]
                    found += [(sc, x, y, d, t) for t, kind in gets if kind == k]
    count = 3 * n + 17
    assert len(found) >= count, len(found)
    order = np.random.RandomState(4).permutation(len(found))[:count]
    return pool, np.ascontiguousarray(np.asarray(found, dtype=np.int32)[order]), len(found)


def check_end_on_a_grab(a, ref, grids, specs, teach=True):
    """a (max_timesteps 1, the queue begun without wrap) steps USE every tick: every episode ends on
    the step that grabs its item.  ref: a handle of the same world and pool that is set to each
    tick's expected initial states for observe and teacher; grids: the pool's rows."""
    n, dev, count = a.n_envs, a.device, len(specs)
    C = a.width * a.height
    a.set_episode_queue(torch.as_tensor(specs))
    a.begin_episodes()
    grids = np.asarray(grids).reshape(len(grids), C)
    pool = lambda idx: grids[idx]   # noqa: E731
    cur = np.arange(n)
    use = torch.full((n,), N.USE, dtype=torch.int32, device=dev)
    ticks = (count + n - 1) // n + 1
    final = {}
    for t in range(ticks):
        out = lang_stream_buffers(a, teach)
        a.step_lang_stream(use, tick=t, **out)
        h = host_outputs(out)
        st = {k: v.cpu().numpy() for k, v in a.get_state().items()}
        run = cur >= 0
        nxt = np.where(run & (cur + n < count), cur + n, -1)
        go, out_of = run & (nxt >= 0), run & (nxt < 0)
        e = specs[np.where(run, cur, 0)]
        # every running slot: the episode ends on the grab, with its task satisfied
        assert (h["done"] == 1).all()
        np.testing.assert_array_equal(h["success"][run], 1)
        np.testing.assert_array_equal(h["transition_code"], np.where(run, GRABBED, -1))
        np.testing.assert_array_equal(h["action_record"], np.where(run, N.USE, -1))
        np.testing.assert_array_equal(h["ask_record"], np.where(run, 0, -1))
        np.testing.assert_array_equal(h["episode_end"], np.where(run, cur, -1))
        np.testing.assert_array_equal(h["end_pose"], np.where(run, e[:, 1] | (e[:, 2] << 8) | (e[:, 3] << 16), -1))
        np.testing.assert_array_equal(h["episode_now"], nxt)
        assert int(h["any_live"][0]) == int(go.any())
        # restarted: nothing of the old episode is left
        en = specs[np.where(go, nxt, 0)]
        assert (st["inventory"][go] == 0).all()
        np.testing.assert_array_equal(st["grid"][go], pool(en[go, 0]))
        np.testing.assert_array_equal(st["spec"][go], en[go])
        np.testing.assert_array_equal(st["agent"][go], np.concatenate([en[go, 1:4], np.ones((go.sum(), 1), int)], 1))
        # run out: the slot keeps the grabbed item and the cleared cell, frozen
        for i in np.nonzero(out_of)[0]:
            kind = ref.config.task[int(e[i, 4])].arg_kind
            assert st["inventory"][i, kind] == 1 and st["inventory"][i].sum() == 1
            cell = (e[i, 1] + _DX[e[i, 3]]) * a.height + e[i, 2] + _DY[e[i, 3]]
            expect = pool(e[i:i + 1, 0])[0].copy()
            assert expect[cell] == kind
            expect[cell] = 0
            np.testing.assert_array_equal(st["grid"][i], expect)
            assert st["agent"][i, 3] == 0
            final[i] = (st["inventory"][i].copy(), st["grid"][i].copy(), st["agent"][i].copy())
        for i, (inv, grid, agent) in final.items():        # and stays so
            assert (st["inventory"][i] == inv).all() and (st["grid"][i] == grid).all() and (st["agent"][i] == agent).all()
        # the obs row and the label of a restarted slot: its new initial state's
        if go.any():
            idx = np.nonzero(go)[0]
            ref.reset(*[np.resize(en[idx][:, j], ref.n_envs) for j in range(5)])
            rows = ref.empty_obs()
            ref.observe(obs=rows)
            assert torch.equal(out["obs"][torch.as_tensor(idx, device=dev)].cpu(), rows[:len(idx)].cpu()), t
            if teach:
                np.testing.assert_array_equal(h["labels"][idx], ref.teacher()[0].cpu().numpy()[:len(idx)])
        if teach:
            assert (h["labels"][~run] == -1).all()
        cur = nxt
    assert (cur < 0).all() and len(final) == n
    ended, steps = a.stats().cpu().numpy()[1:]
    assert ended == count and steps == count
    assert a.stats().cpu().numpy()[0] == count


def turned_away_faces_other(grids, cfg, W, H, spec):
    """Whether, after the action opposite to its direction (a move away, or a turn where that cell is
    taken), the pose of `spec` faces a cell that does not hold its task's kind."""
    sc, x, y, d, t = (int(v) for v in spec)
    g = np.asarray(grids).reshape(len(grids), W, H)[sc]
    ox, oy = x - _DX[d], y - _DY[d]
    fx, fy = (ox - _DX[d], oy - _DY[d]) if g[ox, oy] == 0 else (ox, oy)
    return g[fx, fy] != cfg.task[t].arg_kind


OPPOSITE = (N.UP, N.DOWN, N.RIGHT, N.LEFT)      # of DOWN, UP, LEFT, RIGHT


def check_turn_away_times_out(a, specs):
    """a (max_timesteps 2) on a queue of n poses that face their item: the opposite action, then
    USE.  The second step is the ending one; it grabs nothing and the episode fails by timeout."""
    n, dev = a.n_envs, a.device
    assert len(specs) == n
    a.set_episode_queue(torch.as_tensor(specs))
    a.begin_episodes()
    out = lang_stream_buffers(a)
    away = np.asarray(OPPOSITE, dtype=np.int32)[specs[:, 3]]
    a.step_lang_stream(torch.as_tensor(away, device=dev), tick=0, **out)
    h = host_outputs(out)
    assert (h["done"] == 0).all() and (h["success"] == -1).all() and (h["episode_end"] == -1).all()
    np.testing.assert_array_equal(h["episode_now"], np.arange(n))
    pose = a.get_state(fields=("agent",))["agent"].cpu().numpy()
    out = lang_stream_buffers(a)
    a.step_lang_stream(torch.full((n,), N.USE, dtype=torch.int32, device=dev), tick=1, **out)
    h = host_outputs(out)
    assert (h["done"] == 1).all() and (h["action_record"] == N.USE).all()
    np.testing.assert_array_equal(h["success"], 0)
    np.testing.assert_array_equal(h["episode_end"], np.arange(n))
    np.testing.assert_array_equal(h["end_pose"], pose[:, 0] | (pose[:, 1] << 8) | (pose[:, 2] << 16))
    assert (h["episode_now"] == -1).all() and int(h["any_live"][0]) == 0
    assert a.stats().cpu().tolist() == [0, n, 2 * n]
    a.check()
