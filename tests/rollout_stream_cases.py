"""Shared by tests/test_rollout_stream_cpu.py and tests/test_gpu_rollout_stream.py:
craft_rollout_stream (K ticks per launch on the episode queue) against the loop of
craft_step_stream ticks it must equal, launch by launch, and what such a run has to exercise."""
import numpy as np
import torch

from psketch_amd import _native as N
from tests.helpers import RECT_SHAPES, make_tables, rect_world
from tests.stream_cases import T_MAX, Coverage, draw_actions, queue_inputs

LAUNCHES = (7, 7, 7, 7, 2)           # 30 ticks
RINGS = ("obs", "reward", "done", "success", "episode_end", "end_pose", "episode_now")


def ring_buffers(sim, ring):
    """Every output ring of rollout_stream, filled alike on every simulator."""
    n, dev = sim.n_envs, sim.device
    return {"obs": torch.zeros((ring, n, sim.n_features), dtype=sim.obs_dtype, device=dev),
            "reward": torch.zeros((ring, n), dtype=torch.float32, device=dev),
            "done": torch.zeros((ring, n), dtype=torch.uint8, device=dev),
            "success": torch.zeros((ring, n), dtype=torch.int8, device=dev),
            "episode_end": torch.zeros((ring, n), dtype=torch.int32, device=dev),
            "end_pose": torch.zeros((ring, n), dtype=torch.int32, device=dev),
            "episode_now": torch.zeros((ring, n), dtype=torch.int32, device=dev)}


class LaunchCoverage(Coverage):
    """Coverage, and what only a K-tick launch can get wrong: ends on consecutive ticks (both
    parity buffers reload), two restarts of one slot inside a launch, a restart that stays on its
    scenario and one that leaves it, a slot that runs out before the last launch."""

    def __init__(self, specs, n, wrap):
        super().__init__(specs, n, wrap)
        self.prev_ended = np.zeros(n, bool)
        self.in_launch = np.zeros(n, int)
        self.consecutive = self.twice = self.same_scenario = self.other_scenario = self.out_early = 0

    def begin_launch(self, last):
        self.in_launch[:] = 0
        self.last = last

    def tick(self, acts, out):
        super().tick(acts, out)
        end, now = out["episode_end"], out["episode_now"]
        ended = end >= 0
        moved = ended & (now >= 0)
        self.consecutive += int((ended & self.prev_ended).sum())
        self.prev_ended = ended
        self.in_launch += moved
        self.twice += int((moved & (self.in_launch == 2)).sum())
        same = self.specs[end[moved], 0] == self.specs[now[moved], 0]
        self.same_scenario += int(same.sum())
        self.other_scenario += int((~same).sum())
        if not self.last:
            self.out_early += int((ended & (now < 0)).sum())

    def check(self):
        super().check()
        assert self.consecutive > 0, "no slot's episodes ended on two consecutive ticks"
        assert self.twice > 0, "no slot restarted twice within one launch"
        assert self.same_scenario > 0 and self.other_scenario > 0, "restarts all on / all off their scenario"
        if not self.wrap:
            assert self.out_early > 0, "no slot ran out before the last launch"


def assert_same(a, b, ra, rb, what):
    """Every ring slot, get_state() (spec included), stats() and check() of simulators a and b."""
    for k in RINGS:
        assert torch.equal(ra[k].cpu(), rb[k].cpu()), f"{k} {what}"
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k].cpu(), sb[k].cpu()), f"{k} {what}"
    np.testing.assert_array_equal(a.stats().cpu().numpy(), b.stats().cpu().numpy(), err_msg=what)
    a.check()
    b.check()


def step_ticks(b, rb, ring, t0, k, acts, seed, cov=None):
    """Ticks t0 .. t0 + k - 1 of simulator b as step_stream(teach=False) calls into ring slots
    t % ring; acts: [k, n] host actions or None for the hashed draw."""
    n = b.n_envs
    rec = torch.empty(n, dtype=torch.int32, device=b.device)
    for j in range(k):
        r = (t0 + j) % ring
        b.step_stream(None if acts is None else torch.as_tensor(acts[j], device=b.device), seed=seed,
                      tick=t0 + j, action_record=rec, **{name: rb[name][r] for name in RINGS})
        if cov is not None:
            cov.tick(None, {"episode_end": rb["episode_end"][r].cpu().numpy(),
                            "episode_now": rb["episode_now"][r].cpu().numpy(),
                            "action_record": rec.cpu().numpy()})


def run_rollout_against_steps(a, b, specs, wrap, ring, given, coverage=True, seed=9, others=()):
    """Simulator a runs rollout_stream in launches of LAUNCHES ticks, simulator b (and every
    simulator of `others`, which also run rollout_stream) the same ticks: b one step_stream at a
    time into the same ring slots.  given: True (drawn actions), False (the hashed draw) or
    "alternate" (by launch).  After every launch everything must be equal.  The coverage comes
    from b's outputs alone."""
    n = a.n_envs
    sims = (a, b) + tuple(others)
    for s in sims:
        s.set_episode_queue(torch.as_tensor(specs))
    first = [s.empty_obs() for s in sims]
    for s, o in zip(sims, first):
        s.begin_episodes(wrap=wrap, obs=o)
    rings = [ring_buffers(s, ring) for s in sims]
    cov = LaunchCoverage(specs, n, wrap)
    rng = np.random.RandomState(3)
    t0 = 0
    for li, k in enumerate(LAUNCHES):
        use_given = given if given in (True, False) else li % 2 == 0
        acts = np.stack([draw_actions(rng, n) for _ in range(k)]) if use_given else None
        cov.begin_launch(li == len(LAUNCHES) - 1)
        for s, r in zip(sims, rings):
            if s is b:
                step_ticks(b, r, ring, t0, k, acts, seed, cov)
            else:
                s.rollout_stream(k, seed=seed, tick0=t0,
                                 actions=None if acts is None else torch.as_tensor(acts).to(s.device), **r)
        for s, r in zip(sims, rings):
            if s is not b:
                assert_same(s, b, r, rings[1], f"after launch {li} ({'given' if use_given else 'hashed'})")
        t0 += k
    if not wrap:
        last = (t0 - 1) % ring
        assert (rings[1]["episode_now"][last].cpu().numpy() == -1).all(), "the pass did not end"
    if coverage:
        cov.check()
    return cov


# world, W, H, n, tile (craft_sim_tune's tile_envs on the HIP side, 0 = default), obs format, ring,
# queue seed: 72 = two 32-env tiles and 8, 40 = two 16-env tiles and 8 (or a 32-env tile and 8).
# Every row meets LaunchCoverage.check() with its seed, with and without wrap
# (tests/test_rollout_stream_cpu.py checks that on the CPU variant).
W12, W12_5, W8 = "craft_medium_12x12", "craft_medium_12x12_w5", "craft_medium"
W15_7 = rect_world(15, 15, 7)
R7X13 = rect_world(*RECT_SHAPES["r7x13"])
ROWS = [
    (W12, 12, 12, 72, 0, "f32", 3, 11),
    (W12, 12, 12, 72, 0, "bf16", 1, 11),
    (W12, 12, 12, 72, 0, "u8", 30, 11),
    (W12, 12, 12, 40, 16, "f32", 3, 11),
    (W12_5, 12, 12, 72, 0, "f32", 3, 11),
    (W15_7, 15, 15, 40, 0, "f32", 3, 11),
    (W8, 8, 8, 70, 0, "f32", 3, 11),
    (R7X13, 7, 13, 40, 0, "f32", 3, 11)]
ROW_IDS = [f"{w if isinstance(w, str) else f'{W}x{H}'}-{n}-{fmt}-ring{ring}" + (f"-tile{tile}" if tile else "")
           for w, W, H, n, tile, fmt, ring, seed in ROWS]


def row_sims(row, make_a, make_b, others=()):
    """The row's queue and one simulator per factory(world, n, pool, max_timesteps=), each in the
    row's obs format."""
    world, W, H, n, tile, fmt, ring, seed = row
    pool, specs = queue_inputs(world, W, n, seed=seed, H=H)
    sims = [f(world, n, pool, max_timesteps=T_MAX) for f in (make_a, make_b) + tuple(others)]
    for s in sims:
        s.set_obs_format(fmt)
        if tile and not s._cpu:
            s.tune(tile_envs=tile, obs_store=2)      # (2: the store policy of an untuned handle)
    return specs, sims


def many_clears_case(world="craft_medium_12x12", n=72, T=30):
    """Two hand-made 12x12 scenarios (a boundary ring and seven wood cells in a row, at y = 5 and
    at y = 6), a queue whose slot i alternates between them, and [T, n] actions: slot i repeats
    [USE, RIGHT] x (i % 7), STOP, so that its episodes clear 0..6 cells and then STOP onto the
    other scenario: from four clears on, a restart with an overflowed cleared-cell list."""
    params, cb, tm, cfg = make_tables(world)
    wood, boundary = cb.index["wood"], cb.index["boundary"]
    grids = np.zeros((2, 12, 12), dtype=np.uint8)
    grids[:, 0, :] = grids[:, -1, :] = grids[:, :, 0] = grids[:, :, -1] = boundary
    grids[0, 2:9, 5] = wood
    grids[1, 2:9, 6] = wood
    task = tm["get[wood]"].id
    count = (T + 2) * n                                  # no slot runs out: slot 0 ends one episode per tick
    scen = (np.arange(count) // n) % 2
    specs = np.stack([scen, np.ones(count), 5 + scen, np.full(count, N.RIGHT), np.full(count, task)], 1)
    acts = np.empty((T, n), dtype=np.int32)
    for i in range(n):
        script = [N.USE, N.RIGHT] * (i % 7) + [N.STOP]
        acts[:, i] = [script[t % len(script)] for t in range(T)]
    return grids, np.ascontiguousarray(specs.astype(np.int32)), acts, wood
