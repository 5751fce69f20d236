"""Shared by tests/test_rollout_replay_cpu.py and tests/test_gpu_rollout_replay.py:
craft_rollout_replay (K ticks per launch on the episode queue, every slot's action read from the
installed tape) against the loop of craft_step_stream ticks it must equal.  The reference for the
actions is written out here in numpy, independent of both libraries' tape code: before each tick
every slot's action comes from a host copy of the tape, the previous tick's episode_now and
get_state()'s timer."""
import numpy as np
import torch

from psketch_amd import _native as N
from tests.rollout_stream_cases import (LAUNCHES, RINGS, LaunchCoverage, assert_same, many_clears_case,
                                        ring_buffers, step_ticks)
from tests.stream_cases import T_MAX

# the tape seed of each row of rollout_stream_cases.ROWS: with it the step loop's outputs meet
# LaunchCoverage.check(), with and without wrap (tests/test_rollout_replay_cpu.py confirms it)
TAPE_SEEDS = (21, 21, 21, 21, 21, 21, 21, 21)
TAPE_OUTS = ("step_now", "action_next")


def pad_rows(rows, T):
    """Action sequences as the int32 [count, T] array craft_episode_actions takes, -1 padded."""
    out = np.full((len(rows), T), -1, dtype=np.int32)
    for e, r in enumerate(rows):
        out[e, :len(r)] = r
    return out


def draw_tape(count, seed, T=T_MAX):
    """One recorded sequence per queue entry: lengths uniform in 1..T, non-final actions in 0..4,
    a row of length T ends in STOP with probability 1/2 (else it times out), shorter rows end in
    STOP."""
    rng = np.random.RandomState(seed)
    rows = []
    for _ in range(count):
        k = int(rng.randint(1, T + 1))
        r = rng.randint(0, 5, size=k)
        if k < T or rng.rand() < 0.5:
            r[-1] = N.STOP
        rows.append(r.astype(np.int32))
    return rows


def rule_action(tape, cur, timer, T):
    """The contract's rule in numpy: tape [count, T] (-1 padded), cur / timer [n] before the tick.
    p = T - timer; tape[cur][p] for 0 <= p < T on a slot with an entry, -1 padding as STOP; STOP
    for any other p."""
    p = T - timer
    a = np.full(len(cur), N.STOP, dtype=np.int32)
    ok = (cur >= 0) & (p >= 0) & (p < T)
    a[ok] = tape[cur[ok], p[ok]]
    a[a < 0] = N.STOP
    return a


def timers(sim):
    return sim.get_state(fields=("agent",))["agent"][:, 3].cpu().numpy().astype(np.int64)


def replay_buffers(sim, ring):
    r = ring_buffers(sim, ring)
    for k in TAPE_OUTS:
        r[k] = torch.full((ring, sim.n_envs), -7, dtype=torch.int32, device=sim.device)
    return r


class StepLoop:
    """Simulator b as the all-step loop: one step_stream per tick into ring slots t % ring, fed
    the numpy rule's actions (or the hashed draw), keeping what the rule needs (each slot's cursor
    from the last episode_now) and what the two new outputs must be after every tick."""

    def __init__(self, b, tape, ring, T, cov=None):
        self.b, self.tape, self.ring, self.T, self.cov = b, tape, ring, T, cov
        n = b.n_envs
        self.rb = ring_buffers(b, ring)
        self.cur = np.arange(n, dtype=np.int64)          # begin_episodes(first=0): slot i on entry i
        self.exp = {k: np.full((ring, n), -7, dtype=np.int32) for k in TAPE_OUTS}
        self.acts = []                                   # every tick's actions (None: hashed)

    def ticks(self, t0, k, hashed_seed=None):
        """Ticks t0 .. t0 + k - 1; returns the [k, n] actions fed (None for the hashed draw)."""
        fed = []
        for j in range(k):
            r = (t0 + j) % self.ring
            acts = None if hashed_seed is not None else rule_action(self.tape, self.cur, timers(self.b), self.T)
            step_ticks(self.b, self.rb, self.ring, t0 + j, 1, None if acts is None else acts[None],
                       hashed_seed or 0, self.cov)
            now = self.rb["episode_now"][r].cpu().numpy().astype(np.int64)
            self.cur = now                               # (-1: frozen; a running slot's is its cursor)
            after = timers(self.b)
            self.exp["step_now"][r] = np.where(now < 0, -1, self.T - after)
            self.exp["action_next"][r] = np.where(now < 0, -1, rule_action(self.tape, now, after, self.T))
            fed.append(acts)
            self.acts.append(acts)
        return None if hashed_seed is not None else np.stack(fed)


def assert_replay_same(s, loop, rs, what, rows=None):
    """Simulator s (its rings rs) against the step loop: every ring, get_state(), stats() and
    check(), and the two new outputs against the numpy rule (rows: the ring slots the launch
    wrote, default all)."""
    assert_same(s, loop.b, rs, loop.rb, what)
    for k in TAPE_OUTS:
        got = rs[k].cpu().numpy()
        sel = slice(None) if rows is None else rows
        np.testing.assert_array_equal(got[sel], loop.exp[k][sel], err_msg=f"{k} {what}")


def begin(sims, specs, tape, wrap):
    for s in sims:
        s.set_episode_queue(torch.as_tensor(specs))
        s.set_episode_actions(torch.as_tensor(tape))
    first = [s.empty_obs() for s in sims]
    for s, o in zip(sims, first):
        s.begin_episodes(wrap=wrap, obs=o)
    for o in first[1:]:
        assert torch.equal(first[0].cpu(), o.cpu())


def run_replay_against_steps(a, b, specs, tape, wrap, ring, coverage=True, others=(), launches=LAUNCHES,
                             prepare=None, ends=True):
    """Simulator a (and every simulator of `others`) runs rollout_replay in launches of `launches`
    ticks, simulator b the same ticks one step_stream at a time with the numpy rule's actions.
    After every launch everything must be equal.  prepare(sim): called on every simulator after
    begin_episodes; ends: without wrap the pass must be over at the end.  Returns the StepLoop
    (its coverage from b's outputs alone)."""
    n, T = a.n_envs, a.config.max_timesteps
    sims = (a, b) + tuple(others)
    begin(sims, specs, tape, wrap)
    if prepare is not None:
        for s in sims:
            prepare(s)
    cov = LaunchCoverage(specs, n, wrap)
    loop = StepLoop(b, tape, ring, T, cov)
    rings = {id(s): replay_buffers(s, ring) for s in sims if s is not b}
    t0 = 0
    for li, k in enumerate(launches):
        cov.begin_launch(li == len(launches) - 1)
        loop.ticks(t0, k)
        for s in sims:
            if s is not b:
                s.rollout_replay(k, tick0=t0, **rings[id(s)])
                assert_replay_same(s, loop, rings[id(s)], f"after launch {li}")
        t0 += k
    if ends and not wrap:
        last = (t0 - 1) % ring
        assert (loop.rb["episode_now"][last].cpu().numpy() == -1).all(), "the pass did not end"
    if coverage:
        cov.check()
    return loop


def run_mixed(a, b, specs, tape, ring=30):
    """On simulator a: a rollout_replay launch, three step_stream ticks fed host-computed tape
    actions, a rollout_stream launch with the hashed draw, rollout_replay again; on b the all-step
    loop.  The replay launch after the hashed one picks its actions up from (cursor, timer)
    mid-episode."""
    T = a.config.max_timesteps
    begin((a, b), specs, tape, True)                     # (wrap: no slot runs out before the last launch)
    loop = StepLoop(b, tape, ring, T)
    ra = replay_buffers(a, ring)
    seed = 9
    t0 = 0
    a.rollout_replay(7, tick0=t0, **ra)
    loop.ticks(t0, 7)
    assert_replay_same(a, loop, ra, "after the first replay launch", rows=slice(0, 7))
    t0 = 7
    acts = loop.ticks(t0, 3)
    step_ticks(a, ra, ring, t0, 3, acts, 0)
    assert_same(a, b, ra, loop.rb, "after the three step_stream ticks")
    t0 = 10
    a.rollout_stream(5, seed=seed, tick0=t0, **{k: ra[k] for k in RINGS})
    loop.ticks(t0, 5, hashed_seed=seed)
    assert_same(a, b, ra, loop.rb, "after the hashed rollout_stream launch")
    # not vacuous: the hashed launch left slots in the middle of an episode
    mid = (loop.cur >= 0) & (timers(b) < T)
    assert mid.sum() > a.n_envs // 4
    t0 = 15
    a.rollout_replay(7, tick0=t0, **ra)
    loop.ticks(t0, 7)
    assert_replay_same(a, loop, ra, "after the second replay launch", rows=slice(15, 22))
    return loop


def timer_rule_case(a, b, specs, tape, others=()):
    """set_state puts three running slots at timer 0, max_timesteps + 3 and 2: the next launch's
    actions, step_now and action_next follow the rule (STOP, STOP, tape[c][max_timesteps - 2])."""
    T = a.config.max_timesteps
    tm = np.asarray([0, T + 3, 2])

    def prepare(s):
        st = s.get_state(slots=torch.arange(3, dtype=torch.int32))
        agent = st["agent"].cpu().numpy().copy()
        agent[:, 3] = tm
        s.set_state(st["spec"], torch.as_tensor(agent), slots=torch.arange(3, dtype=torch.int32))

    loop = run_replay_against_steps(a, b, specs, tape, False, 3, coverage=False, others=others, launches=(4, 3),
                                    prepare=prepare, ends=False)
    first = loop.acts[0]
    assert first[0] == N.STOP and first[1] == N.STOP
    assert tape[2, T - 2] >= 0 and tape[2, T - 2] != N.STOP and first[2] == tape[2, T - 2]
    return loop


def many_clears_tape(n, count, T):
    """many_clears_case's actions as a tape: entry e of slot e % n holds [USE, RIGHT] x (slot % 7)
    then STOP."""
    return pad_rows([[N.USE, N.RIGHT] * ((e % n) % 7) + [N.STOP] for e in range(count)], T)


def wrap_epochs_case(sim, pool_specs, seed=5):
    """A queue of exactly 2n entries under CRAFT_QUEUE_WRAP whose every slot's two rows are P = 8
    ticks long together (rows of 2..6 actions; a row of max_timesteps = 6 never STOPs, a shorter
    one ends in its STOP): ticks t and t + P must produce equal rows for every slot."""
    n, T, P = sim.n_envs, sim.config.max_timesteps, 8
    assert T == 6
    specs = np.ascontiguousarray(pool_specs[:2 * n])
    rng = np.random.RandomState(seed)
    l1 = rng.randint(2, 7, size=n)
    rows = []
    for k in np.concatenate([l1, P - l1]):
        r = rng.randint(0, 5, size=k)
        if k < T:
            r[-1] = N.STOP
        rows.append(r)
    tape = pad_rows(rows, T)
    begin((sim,), specs, tape, True)
    ring = 2 * P
    r = replay_buffers(sim, ring)
    sim.rollout_replay(5, tick0=0, **r)
    sim.rollout_replay(ring - 5, tick0=5, **r)
    sim.check()
    for k in RINGS + TAPE_OUTS:
        x = r[k].cpu()
        assert torch.equal(x[:P], x[P:]), k
    end = r["episode_end"].cpu().numpy()
    assert ((end[:P] >= 0).sum(0) == 2).all()             # every slot ended both its rows in a period
    assert (r["action_next"].cpu().numpy() >= 0).all()
    return tape
