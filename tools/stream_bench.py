#!/usr/bin/env python
"""craft_step_stream (the episode queue's tick, wrap on) against the tick it extends: the one-tile
craft_step_ex / craft_step_teach(kernel=1) with CRAFT_STEP_AUTORESET.  The same phases over the
same bytes; the stream tick adds one cursor load per env, three int32 outputs per env, and in the
lanes that restart (about one in six per tick under the hashed draw: STOP is one of six actions)
the queue entry and a reload of the grid row from the new scenario's pool row.

At 65,536 envs of 12x12 worlds with 3x3 and 5x5 windows, with and without the teacher, hashed
actions, timed with device events around `--steps` back-to-back launches that rewrite one
observation buffer (a trainer's loop), the sides alternating run by run on one device.

The yardstick is the existing tick built from the PARENT commit: `--tree DIR` imports the package
(and its built library) from another checkout and times only that tick (`--sides step`), so a
caller alternates invocations of the two trees on one box; without it both sides come from this
tree.  Prints one JSON line per (window, teacher) case: the per-run microseconds per tick of each
side, medians and spread (max - min of a side's runs).

Two more sides time the language protocol the same way: `lang` (craft_step_lang, which has no
auto-reset: its envs are reset before every timed run, outside the timed window, and --steps stays
inside max_timesteps, as in tools/lang_bench.py) and `lang_stream` (craft_step_lang_stream, the
same tick on the queue, wrap on).  With both pairs a line also carries lang_stream - lang and
lang_stream - stream beside stream - step, the gap the queue already costs the imitation tick.
Under the hashed draw the lang side's envs freeze as they STOP while lang_stream's restart and
run on, so lang_stream - lang is an upper bound of what the queue adds.  `--actions nostop` gives
every side the same work instead: a given action buffer without STOP, so that within a timed
window no episode ends on the lang side and, but for the tick on which every timer runs out at
once, none restarts on the queued sides; the differences are then the modes' fixed costs.

Two K-tick sides time the launches that keep a tile on chip between ticks: `rollout`
(craft_rollout with CRAFT_STEP_AUTORESET: every slot replays its own spec) and `rollout_stream`
(craft_rollout_stream, the same launch on the queue, wrap on); `rollout_split` is craft_rollout
tuned to rollout_stream's launch shape (32-env tiles, 512 threads: the default at 3x3 windows
only), so that at wider windows the queue's cost can be told from the shape's.  A timed run is `--launches`
back-to-back launches of `--ticks` ticks each into an observation ring of `--ring` slots (the
one-tick sides keep rewriting one buffer unless `--one-tick-ring` gives them the same ring, a
slot per tick), microseconds per tick = time / (launches x ticks); they
run without the teacher only.  rollout_stream - rollout is what the queue costs the K-tick launch
(`--actions nostop`: no restart but the one tick on which every timer runs out, so the variant's
fixed cost), rollout_stream - stream what the K-tick launch buys a queue workload.

Two more K-tick sides carry the teacher: `rollout_teach` (craft_rollout_teach, every slot on its own
spec) and `rollout_teach_stream` (craft_rollout_teach_stream, the same launch on the queue, wrap
on).  They run in the teacher pass only, writing the observation ring and a labels ring, beside the
`stream` side's per-tick craft_step_stream(label_out) (give it the ring with --one-tick-ring).
rollout_teach_stream - rollout_teach is what the queue costs the launch, rollout_teach_stream -
stream what the launch buys a queue workload.  `--actions label` makes every slot act on its label
(make_data's demonstrations): the K-tick sides with label_actions, each launch fed the labels of
the tick before it, the stream side with ref_actions = the last tick's labels and behavior_clone
all ones; only these three sides take it.

    python tools/stream_bench.py [--envs 65536] [--steps 32] [--runs 9]
                                 [--sides step,stream,lang,lang_stream,rollout,rollout_split,rollout_stream,
                                          rollout_teach,rollout_teach_stream]
                                 [--actions hashed|nostop|label] [--ticks 20] [--launches 8] [--ring 16]
                                 [--one-tick-ring] [--worlds w3,w5] [--tree DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch


QUEUED = ("stream", "lang_stream", "rollout_stream", "rollout_teach_stream")
KTICK = ("rollout", "rollout_split", "rollout_stream")
KTICK_TEACH = ("rollout_teach", "rollout_teach_stream")
ALL_SIDES = ("step", "stream", "lang", "lang_stream") + KTICK + KTICK_TEACH


def make(P, world, n, pool, specs, queue, side):
    sim = P.CraftSim(world, n_envs=n, device=0, pool_capacity=len(pool))
    sim.load_pool(pool)
    sim.tune_teach(kernel=1)
    if side == "rollout_split":                  # craft_rollout in rollout_stream's launch shape
        sim.tune(tile_envs=32, obs_store=2)
        sim.tune_rollout(0, 512)
    if side in QUEUED:
        sim.set_episode_queue(torch.as_tensor(queue))
        sim.begin_episodes(wrap=True)
    else:
        sim.reset(*specs)
    return sim


def timed_launches(sim, side, bufs, tick0, ticks, launches):
    """A K-tick side: `launches` launches of `ticks` ticks, microseconds per tick."""
    fn = sim.rollout_stream if side == "rollout_stream" else sim.rollout
    kw = dict(seed=5, actions=bufs["ktick_actions"], obs=bufs["ring"])
    fn(ticks, tick0=tick0, **kw)                                     # (warm)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for l in range(1, launches + 1):
        fn(ticks, tick0=tick0 + l * ticks, **kw)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (launches * ticks)


def timed_teach_launches(sim, side, bufs, tick0, ticks, launches, label):
    """A teacher K-tick side: `launches` launches of `ticks` ticks into the observation and labels
    rings, microseconds per tick.  label: every slot acts on its label, each launch fed the last
    labels the launch before it wrote (a copy into label_in: the ring slot is rewritten)."""
    fn = sim.rollout_teach_stream if side == "rollout_teach_stream" else sim.rollout_teach
    ring = bufs["label_ring"]
    kw = dict(seed=5, actions=bufs["ktick_actions"], obs=bufs["ring"], labels=ring)
    cur = bufs["label_in"]
    if label:
        cur.copy_(sim.teacher()[0])
        kw.update(label_actions=True, label_in=cur)

    def launch(t0):
        fn(ticks, tick0=t0, **kw)
        if label:
            cur.copy_(ring[(t0 + ticks - 1) % ring.shape[0]])
    launch(tick0)                                                    # (warm)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for l in range(1, launches + 1):
        launch(tick0 + l * ticks)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (launches * ticks)


def timed_label_stream(sim, steps, bufs, tick0):
    """The stream side under --actions label: craft_step_stream(label_out) per tick, every slot
    acting on the labels of the tick before, labels into the ring's slot of the tick."""
    ring, obs_ring = bufs["label_ring"], bufs.get("one_tick_ring")
    R = ring.shape[0]
    kw = dict(done=bufs["done"], behavior_clone=bufs["ones"], episode_end=bufs["end"], end_pose=bufs["pose"],
              episode_now=bufs["now"])
    ring[(tick0 - 1) % R].copy_(sim.teacher()[0])

    def tick(t):
        sim.step_stream(None, seed=5, tick=t, obs=bufs["obs"] if obs_ring is None else obs_ring[t % obs_ring.shape[0]],
                        ref_actions=ring[(t - 1) % R], labels=ring[t % R], **kw)
    tick(tick0)                                                      # (warm)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(tick0 + 1, tick0 + steps + 1):
        tick(t)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def timed(sim, steps, side, bufs, tick0, specs):
    kw = dict(obs=bufs["obs"], done=bufs["done"], labels=bufs["labels"])
    if side in QUEUED:
        fn = sim.step_stream if side == "stream" else sim.step_lang_stream
        kw.update(episode_end=bufs["end"], end_pose=bufs["pose"], episode_now=bufs["now"])
    elif side == "lang":
        sim.reset(*specs)                        # no auto-reset in this protocol: fresh episodes per run
        fn = sim.step_lang
    else:
        fn = sim.step
        kw["autoreset"] = True
    acts = bufs["actions"]                                           # None: the hashed draw
    fn(acts, seed=5, tick=tick0, **kw)                               # (warm)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ring = bufs.get("one_tick_ring")                                 # --one-tick-ring: tick t writes slot t % ring
    for t in range(tick0 + 1, tick0 + steps + 1):
        if ring is not None:
            kw["obs"] = ring[t % ring.shape[0]]
        fn(acts, seed=5, tick=t, **kw)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--sides", default="step,stream")
    ap.add_argument("--actions", default="hashed", choices=("hashed", "nostop", "label"))
    ap.add_argument("--ticks", type=int, default=20, help="ticks per launch of the K-tick sides")
    ap.add_argument("--launches", type=int, default=8, help="launches per timed run of the K-tick sides")
    ap.add_argument("--ring", type=int, default=16, help="observation ring slots of the K-tick sides")
    ap.add_argument("--one-tick-ring", action="store_true",
                    help="the one-tick sides write the K-tick sides' ring too, a slot per tick")
    ap.add_argument("--worlds", default="w3,w5")
    ap.add_argument("--tree", default=None, help="checkout to import psketch_amd from (default: this one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    import psketch_amd as P
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs a GPU")
    sides = [s for s in a.sides.split(",") if s]
    if not set(sides) <= set(ALL_SIDES):
        raise SystemExit("--sides: " + ", ".join(ALL_SIDES))
    label = a.actions == "label"
    if label and not set(sides) <= {"stream"} | set(KTICK_TEACH):
        raise SystemExit("--actions label: sides stream, rollout_teach, rollout_teach_stream only")
    n = a.envs
    lines = []
    worlds = {"w3": ("craft_medium_12x12", 12), "w5": ("craft_medium_12x12_w5", 12)}
    for world, W in (worlds[w] for w in a.worlds.split(",") if w):
        probe = P.CraftSim(world, n_envs=64, device=0, pool_capacity=1)
        if "lang" in sides and a.steps + 1 >= probe.config.max_timesteps:
            raise SystemExit("--steps must stay inside max_timesteps for the lang side")
        pool, _, _ = P.sample_scenarios(probe.params, probe.cookbook, 123, 256)
        tasks = [t.id for t in probe.task_manager.dataset_tasks()]
        queue = np.stack(P.synthetic_specs(pool, W, W, 2 * n + 17, 0, seed=0, task_ids=tasks), 1).astype(np.int32)
        specs = [torch.as_tensor(np.ascontiguousarray(queue[:n, j]), device="cuda") for j in range(5)]
        sims = {k: make(P, world, n, pool, specs, queue, k) for k in sides}
        i32 = dict(dtype=torch.int32, device="cuda")
        bufs = {"obs": next(iter(sims.values())).empty_obs(), "done": torch.empty(n, dtype=torch.uint8, device="cuda"),
                "end": torch.empty(n, **i32), "pose": torch.empty(n, **i32), "now": torch.empty(n, **i32),
                "actions": (torch.arange(n, **i32) % 5) if a.actions == "nostop" else None}
        if set(sides) & set(KTICK_TEACH) or label:
            bufs["label_ring"] = torch.empty((a.ring, n), **i32)
            bufs["label_in"] = torch.empty(n, **i32)
            bufs["ones"] = torch.ones(n, dtype=torch.uint8, device="cuda")
        if set(sides) & set(KTICK + KTICK_TEACH):
            bufs["ring"] = torch.empty((a.ring, n, bufs["obs"].shape[1]), dtype=bufs["obs"].dtype, device="cuda")
            bufs["ktick_actions"] = (bufs["actions"].repeat(a.ticks, 1).contiguous()
                                     if a.actions == "nostop" else None)
            if a.one_tick_ring:
                bufs["one_tick_ring"] = bufs["ring"]
        for teach in (False, True):
            bufs["labels"] = torch.empty(n, **i32) if teach else None
            run_sides = [k for k in sims if not (teach and k in KTICK) and not (not teach and (k in KTICK_TEACH or label))]
            if not run_sides:
                continue
            us = {k: [] for k in run_sides}
            for r in range(a.runs + 1):          # run 0 warms every side and is dropped
                for k in run_sides:
                    if k in KTICK_TEACH:
                        v = timed_teach_launches(sims[k], k, bufs, r * (a.launches + 1) * a.ticks, a.ticks,
                                                 a.launches, label)
                    elif label:
                        v = timed_label_stream(sims[k], a.steps, bufs, 1 + r * (a.steps + 1))
                    elif k in KTICK:
                        v = timed_launches(sims[k], k, bufs, r * (a.launches + 1) * a.ticks, a.ticks, a.launches)
                    else:
                        v = timed(sims[k], a.steps, k, bufs, r * (a.steps + 1), specs)
                    if r:
                        us[k].append(round(v, 3))
            for s in sims.values():
                s.check()
            line = {"tree": tree, "world": world, "envs": n, "teacher": teach, "actions": a.actions, "steps": a.steps, "runs": a.runs,
                    "ticks": a.ticks, "launches": a.launches, "ring": a.ring,
                    "one_tick_ring": a.one_tick_ring,
                    "us_per_tick": us, "median_us": {k: statistics.median(v) for k, v in us.items()},
                    "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()}}
            med = line["median_us"]
            if set(us) == {"step", "stream"}:
                d = med["stream"] - med["step"]
                line["stream_minus_step_us"] = round(d, 3)
                line["within_spread"] = abs(d) <= max(line["spread_us"].values())
            elif len(us) > 1:
                for hi, lo in (("stream", "step"), ("lang_stream", "lang"), ("lang_stream", "stream"),
                               ("rollout_stream", "rollout"), ("rollout_stream", "rollout_split"),
                               ("rollout_stream", "stream"), ("rollout_teach_stream", "rollout_teach"),
                               ("rollout_teach_stream", "stream")):
                    if hi in med and lo in med:
                        line[f"{hi}_minus_{lo}_us"] = round(med[hi] - med[lo], 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
