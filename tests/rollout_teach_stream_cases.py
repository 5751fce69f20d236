"""Shared by tests/test_rollout_teach_stream_cpu.py and tests/test_gpu_rollout_teach_stream.py:
craft_rollout_teach_stream (K teacher-labelled ticks per launch on the episode queue) against the
loop of craft_step_stream(label_out) ticks its contract names, launch by launch, and what such a
run has to exercise."""
import copy

import numpy as np
import torch

from psketch_amd import _native as N
from psketch_amd import gamedef, sample_scenarios, synthetic_specs
from tests.helpers import make_tables
from tests.rollout_stream_cases import (LAUNCHES, R7X13, RINGS, W8, W12, W12_5, W15_7, LaunchCoverage,
                                        many_clears_case, ring_buffers)
from tests.stream_cases import T_MAX, Coverage, draw_actions, queue_inputs

TEACH_RINGS = RINGS + ("labels", "action_record")
MODES = ("given", "hashed", "bc", "label")


def teach_ring_buffers(sim, ring):
    """Every output ring of rollout_teach_stream, filled alike on every simulator."""
    n, dev = sim.n_envs, sim.device
    out = ring_buffers(sim, ring)
    out["labels"] = torch.zeros((ring, n), dtype=torch.int32, device=dev)
    out["action_record"] = torch.zeros((ring, n), dtype=torch.int32, device=dev)
    return out


def bc_mask(n):
    return (np.random.RandomState(4).rand(n) < 0.5).astype(np.uint8)


def assert_same(a, b, ra, rb, what):
    """Every ring slot, get_state() (spec included), stats() and check() of simulators a and b."""
    for k in TEACH_RINGS:
        assert torch.equal(ra[k].cpu(), rb[k].cpu()), f"{k} {what}"
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k].cpu(), sb[k].cpu()), f"{k} {what}"
    np.testing.assert_array_equal(a.stats().cpu().numpy(), b.stats().cpu().numpy(), err_msg=what)
    a.check()
    b.check()


class TeachCoverage:
    """The mode's coverage conditions, from the step loop's outputs alone: LaunchCoverage for the
    policy and bc modes (bc: also a cloning slot's episode ended on a label STOP), Coverage for
    label actions plus an episode that ended by STOP with success 1."""

    def __init__(self, specs, n, wrap, mode, mask):
        self.mode, self.mask = mode, mask
        self.cov = Coverage(specs, n, wrap) if mode == "label" else LaunchCoverage(specs, n, wrap)
        self.label_stop = self.stop_success = 0
        self.bad_label = 0

    def begin_launch(self, last):
        if self.mode != "label":
            self.cov.begin_launch(last)

    def tick(self, out, prev_labels):
        self.cov.tick(None, out)
        ended, rec = out["episode_end"] >= 0, out["action_record"]
        stop = ended & (rec == N.STOP)
        self.stop_success += int((stop & (out["success"] == 1)).sum())
        if self.mask is not None:
            self.label_stop += int((stop & (self.mask != 0) & (prev_labels == N.STOP)).sum())
        self.bad_label += int((out["labels"] == -2).sum())

    def check(self):
        self.cov.check()
        assert self.bad_label == 0, "a label was -2"
        if self.mode == "bc":
            assert self.label_stop > 0, "no cloning slot's episode ended on a label STOP"
        if self.mode == "label":
            assert self.stop_success > 0, "no episode ended by STOP with success 1"


def mode_args(sim, mode, acts, mask):
    """rollout_teach_stream's action-source arguments for `mode` on `sim`'s device."""
    kw = {}
    if mode in ("given", "bc"):
        kw["actions"] = torch.as_tensor(acts).to(sim.device)
    if mode == "bc":
        kw["behavior_clone"] = torch.as_tensor(mask).to(sim.device)
    if mode == "label":
        kw["label_actions"] = True
    return kw


def step_teach_ticks(b, rb, ring, t0, k, acts, seed, mode, mask, cur, cov=None):
    """The contract's loop on simulator b: ticks t0 .. t0 + k - 1 as step_stream(labels=) calls
    into ring slots t % ring, each fed the labels of the tick before (`cur` first).  Returns the
    last tick's labels."""
    n, dev = b.n_envs, b.device
    feeds = mode in ("bc", "label")
    src = None
    if mode == "bc":
        src = torch.as_tensor(mask).to(dev)
    elif mode == "label":
        src = torch.ones(n, dtype=torch.uint8, device=dev)
    for j in range(k):
        r = (t0 + j) % ring
        prev = cur
        b.step_stream(None if acts is None else torch.as_tensor(acts[j]).to(dev), seed=seed, tick=t0 + j,
                      ref_actions=cur if feeds else None, behavior_clone=src,
                      **{name: rb[name][r] for name in TEACH_RINGS})
        cur = rb["labels"][r].clone()
        if cov is not None:
            out = {name: rb[name][r].cpu().numpy() for name in
                   ("episode_end", "episode_now", "action_record", "success", "labels")}
            cov.tick(out, prev.cpu().numpy())
    return cur


def run_teach_against_steps(a, b, specs, wrap, ring, mode, coverage=True, seed=9, others=(), mask=None,
                            launches=LAUNCHES, cov=None):
    """Simulator a (and every simulator of `others`) runs rollout_teach_stream in launches of
    LAUNCHES ticks, simulator b the contract's step_stream loop into the same ring slots; after
    every launch everything must be equal.  The coverage comes from b's outputs alone."""
    n = a.n_envs
    sims = (a, b) + tuple(others)
    for s in sims:
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes(wrap=wrap)
    rings = [teach_ring_buffers(s, ring) for s in sims]
    if mask is None and mode == "bc":
        mask = bc_mask(n)
    if cov is None:
        cov = TeachCoverage(specs, n, wrap, mode, mask)
    cur = [s.teacher()[0].clone() for s in sims]
    for c in cur[1:]:
        assert torch.equal(c.cpu(), cur[0].cpu())
    rng = np.random.RandomState(3)
    t0 = 0
    for li, k in enumerate(launches):
        acts = np.stack([draw_actions(rng, n) for _ in range(k)]) if mode in ("given", "bc") else None
        cov.begin_launch(li == len(launches) - 1)
        for i, (s, r) in enumerate(zip(sims, rings)):
            if s is b:
                cur[i] = step_teach_ticks(b, r, ring, t0, k, acts, seed, mode, mask, cur[i], cov)
            else:
                s.rollout_teach_stream(k, seed=seed, tick0=t0, label_in=cur[i], **mode_args(s, mode, acts, mask), **r)
                cur[i] = r["labels"][(t0 + k - 1) % ring].clone()
        for s, r in zip(sims, rings):
            if s is not b:
                assert_same(s, b, r, rings[1], f"after launch {li} ({mode})")
        t0 += k
    if coverage:
        cov.check()
    return cov, rings


# world, W, H, n, obs format, ring: 72 = two 32-env tiles and 8 lanes, 40 = two 16-env tiles and 8
# lanes (5x5 and 7x7 windows), 15x15: 8 BFS words, 8x8: 2.  The queue of every row is
# queue_inputs(seed=11); every row runs in every mode, with and without wrap.
ROWS = [
    (W12, 12, 12, 72, "f32", 3),
    (W12, 12, 12, 72, "bf16", 3),
    (W12, 12, 12, 72, "u8", 3),
    (W12, 12, 12, 72, "f32", 1),
    (W12, 12, 12, 72, "f32", 30),
    (W12_5, 12, 12, 40, "f32", 3),
    (W15_7, 15, 15, 40, "f32", 3),
    (W8, 8, 8, 70, "f32", 3),
    (R7X13, 7, 13, 40, "f32", 3)]
ROW_IDS = [f"{w if isinstance(w, str) else f'{W}x{H}'}-{n}-{fmt}-ring{ring}" for w, W, H, n, fmt, ring in ROWS]


def row_sims(row, *factories):
    """The row's queue and one simulator per factory(world, n, pool, max_timesteps=), each in the
    row's obs format."""
    world, W, H, n, fmt, ring = row
    pool, specs = queue_inputs(world, W, n, seed=11, H=H)
    sims = [f(world, n, pool, max_timesteps=T_MAX) for f in factories]
    for s in sims:
        s.set_obs_format(fmt)
    return specs, sims


# ---- the teacher table on and off, after a reload -------------------------------------------------
def many_clears_run(make_sim, table):
    """many_clears_case (restarts after 0..6 clears onto the other scenario) under
    tune_teach(table=): sim a in K-tick launches with given actions, labels and the three queue
    outputs, sim b the step loop.  As the case stands every episode starts facing wood, so no
    label is ever a move; every third pass over the slots therefore starts facing UP instead
    (the label there is RIGHT, and the scripted episode clears one cell fewer).  Returns a's
    rings on the host; what the run exercised is asserted from b's outputs."""
    n, T = 72, 30
    grids, specs, acts, wood = many_clears_case(W12, n, T)
    specs = specs.copy()
    specs[(np.arange(len(specs)) // n) % 3 == 2, 3] = N.UP
    a, b = make_sim(W12, n, grids), make_sim(W12, n, grids)
    for s in (a, b):
        s.tune_teach(table=table)
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes()
    ra, rb = teach_ring_buffers(a, T), teach_ring_buffers(b, T)
    t0 = 0
    cleared = np.zeros(n, int)
    after_many = 0
    for k in LAUNCHES:
        a.rollout_teach_stream(k, tick0=t0, actions=torch.as_tensor(acts[t0:t0 + k]).to(a.device), **ra)
        step_teach_ticks(b, rb, T, t0, k, acts[t0:t0 + k], 0, "given", None, None)
        assert_same(a, b, ra, rb, f"after tick {t0 + k - 1} (table={table})")
        t0 += k
    end, now, lab = (rb[x].cpu().numpy() for x in ("episode_end", "episode_now", "labels"))
    restarted = (end >= 0) & (now >= 0)
    # the cells an episode cleared: its USE actions (every one faces wood), but for the first of
    # an episode that started facing UP
    rec = rb["action_record"].cpu().numpy()
    entry = np.arange(n)
    for t in range(T):
        cleared += rec[t] == N.USE
        many = cleared - (specs[entry, 3] == N.UP) >= 4
        after_many += int((restarted[t] & many).sum())
        cleared[end[t] >= 0] = 0
        entry = np.where(now[t] >= 0, now[t], entry)
    assert after_many > 0, "no slot restarted after >= 4 clears"
    assert ((lab >= 0) & (lab <= 3) & restarted).any(), "no label after a restart is a move"
    return {k: ra[k].cpu() for k in TEACH_RINGS}


# ---- the hint-walk config (the row-synchronous mode) ---------------------------------------------
def hint_walk_inputs(n=72, seed=11):
    """make[ladder] with a hint tree too large for the tabulated walk (tests/
    test_gpu_rollout_teach.py's override), and a shuffled queue of 3n + 17 entries in which it
    is as common as two dataset tasks.  Returns hints, pool, specs and the ladder task's id."""
    hints = copy.deepcopy(gamedef.HINTS)
    hints["make[ladder]"] = ["make[bed]", "make[axe]", "make[shears]", "makeat[workshop2]"]
    params, cb, tm, cfg = make_tables(W12, T_MAX)
    pool, _, _ = sample_scenarios(params, cb, 123, 24)
    from psketch_amd import CraftSim
    tm = CraftSim(W12, n_envs=1, device="cpu", pool_capacity=1, hints=hints).task_manager
    ladder = tm["make[ladder]"].id
    count = 3 * n + 17
    specs = np.stack(synthetic_specs(pool, 12, 12, count, 0, seed=seed,
                                     task_ids=[ladder, ladder] + [t.id for t in tm.dataset_tasks()]), 1).astype(np.int32)
    rng = np.random.RandomState(seed)
    specs = specs[rng.permutation(count)]
    specs[:, 3] = rng.randint(0, 4, size=count)
    return hints, pool, np.ascontiguousarray(specs), ladder


class HintWalkCoverage(TeachCoverage):
    """TeachCoverage's counters without its conditions; instead: some slot restarts from
    make[ladder] onto a tabulated task, and some the other way."""

    def __init__(self, specs, n, wrap, mode, mask, ladder):
        super().__init__(specs, n, wrap, "label", mask)     # (Coverage: no launch bookkeeping)
        self.specs, self.ladder = specs, ladder
        self.off = self.on = 0

    def tick(self, out, prev_labels):
        super().tick(out, prev_labels)
        end, now = out["episode_end"], out["episode_now"]
        moved = (end >= 0) & (now >= 0)
        was = self.specs[end[moved], 4] == self.ladder
        is_ = self.specs[now[moved], 4] == self.ladder
        self.off += int((was & ~is_).sum())
        self.on += int((~was & is_).sum())

    def check(self):
        assert self.off > 0, "no slot restarted from make[ladder] onto a tabulated task"
        assert self.on > 0, "no slot restarted from a tabulated task onto make[ladder]"


def run_hint_walk(make_a, make_b, mode, others=()):
    hints, pool, specs, ladder = hint_walk_inputs()
    sims = [f(W12, 72, pool, max_timesteps=T_MAX, hints=hints) for f in (make_a, make_b) + tuple(others)]
    mask = bc_mask(72) if mode == "bc" else None
    cov = HintWalkCoverage(specs, 72, False, mode, mask, ladder)
    run_teach_against_steps(sims[0], sims[1], specs, False, 3, mode, others=sims[2:], mask=mask, cov=cov)


# ---- mixing the four stream entry points ----------------------------------------------------------
def run_mixed(a, b, specs):
    """Sim a alternates rollout_teach_stream, step_stream, rollout_stream and step_lang_stream
    between launches; sim b runs the same 16 ticks one at a time.  One cursor: states, cursors
    (episode_now) and every ring row equal at the end."""
    n, ring = a.n_envs, 16
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes()
    ra, rb = teach_ring_buffers(a, ring), teach_ring_buffers(b, ring)
    rng = np.random.RandomState(6)
    acts = np.stack([draw_actions(rng, n) for _ in range(ring)])
    da = torch.as_tensor(acts).to(a.device)
    db = torch.as_tensor(acts).to(b.device)
    lang = ("obs", "done", "success", "episode_end", "end_pose", "episode_now")
    mask = bc_mask(n)
    ca, cb = a.teacher()[0].clone(), b.teacher()[0].clone()

    def stream_rings(r, sl):
        return {k: r[k][sl] for k in RINGS}

    # ticks 0-4: the teacher K-tick launch (bc); 5: step_stream; 6-9: rollout_stream; 10:
    # step_lang_stream; 11-15: the teacher K-tick launch again, fed tick 10's labels
    a.rollout_teach_stream(5, tick0=0, actions=da[:5], behavior_clone=torch.as_tensor(mask).to(a.device),
                           label_in=ca, **ra)
    step_teach_ticks(a, ra, ring, 5, 1, acts[5:6], 0, "given", None, None)
    a.rollout_stream(4, tick0=6, actions=da[6:10], **{k: ra[k] for k in RINGS})
    a.step_lang_stream(da[10], tick=10, labels=ra["labels"][10], action_record=ra["action_record"][10],
                       **{k: ra[k][10] for k in lang})
    a.rollout_teach_stream(5, tick0=11, actions=da[11:], behavior_clone=torch.as_tensor(mask).to(a.device),
                           label_in=ra["labels"][10].clone(), **ra)

    step_teach_ticks(b, rb, ring, 0, 5, acts[:5], 0, "bc", mask, cb)
    step_teach_ticks(b, rb, ring, 5, 1, acts[5:6], 0, "given", None, None)
    rec = torch.empty(n, dtype=torch.int32, device=b.device)
    for t in range(6, 10):
        b.step_stream(db[t], tick=t, action_record=rec, **stream_rings(rb, t))
    b.step_lang_stream(db[10], tick=10, labels=rb["labels"][10], action_record=rb["action_record"][10],
                       **{k: rb[k][10] for k in lang})
    step_teach_ticks(b, rb, ring, 11, 5, acts[11:], 0, "bc", mask, rb["labels"][10].clone())
    # ticks 6-9 write no labels / action_record on either side (zeros on both)
    assert_same(a, b, ra, rb, "after the sixteen ticks")
    end = rb["episode_end"].cpu().numpy()
    assert all((end[lo:hi] >= 0).any() for lo, hi in ((0, 5), (5, 6), (6, 10), (10, 11), (11, 16)))


# ---- demonstrations ---------------------------------------------------------------------------------
def demo_split(golden, split):
    g = golden("devtest.npz")
    acts = g[f"{split}_actions"].astype(np.int32)
    pos = g[f"{split}_pos"].astype(np.int32)
    count = len(acts)
    specs = np.stack([g[f"{split}_world"], pos[:, 0], pos[:, 1], np.zeros(count), g[f"{split}_task"]], 1)
    return g[f"{split}_grids"], np.ascontiguousarray(specs.astype(np.int32)), acts


DEMO_TICKS = {"dev": 256, "test": 288}


def check_demonstrations(make_sim, golden, split):
    """rollout.demonstrations over the split on 104 slots: every sequence equals the fixture's,
    every success is 1, and the pass ends within DEMO_TICKS[split] ticks."""
    from psketch_amd import rollout
    grids, specs, acts = demo_split(golden, split)
    sim = make_sim("craft_medium", 104, grids, max_timesteps=40)
    info = rollout.demonstrations(sim, specs, ticks_per_launch=32)
    want_len = (acts >= 0).sum(1)
    np.testing.assert_array_equal(info.length, want_len)
    w = acts.shape[1]
    got = np.full_like(acts, -1)
    got[:, :min(w, info.action_seqs.shape[1])] = info.action_seqs[:, :w]
    np.testing.assert_array_equal(got, acts)
    assert (info.action_seqs[:, w:] == -1).all()
    assert (info.success == 1).all()
    assert info.ticks <= DEMO_TICKS[split], info.ticks
    assert info.actions(0) == [int(x) for x in acts[0][acts[0] >= 0]]
    sim.check()
    return info


def check_demonstrations_time_limit(make_sim, golden):
    """max_timesteps = 5: RolloutError names the first instance longer than 5, and the handle
    runs a valid pass afterwards."""
    import pytest
    from psketch_amd import rollout
    grids, specs, acts = demo_split(golden, "dev")
    length = (acts >= 0).sum(1)
    first = int(np.argmax(length > 5))
    assert length[first] > 5
    sim = make_sim("craft_medium", 104, grids, max_timesteps=5)
    with pytest.raises(rollout.RolloutError, match=rf"instance {first} reached the time limit"):
        rollout.demonstrations(sim, specs, ticks_per_launch=32)
    short = np.nonzero(length <= 5)[0][:150]
    info = rollout.demonstrations(sim, specs[short], ticks_per_launch=8)
    np.testing.assert_array_equal(info.length, length[short])
    assert (info.success == 1).all()
    sim.check()
