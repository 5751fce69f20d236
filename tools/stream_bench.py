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

    python tools/stream_bench.py [--envs 65536] [--steps 32] [--runs 9]
                                 [--sides step,stream,lang,lang_stream] [--actions hashed|nostop]
                                 [--tree DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch


QUEUED = ("stream", "lang_stream")


def make(P, world, n, pool, specs, queue, side):
    sim = P.CraftSim(world, n_envs=n, device=0, pool_capacity=len(pool))
    sim.load_pool(pool)
    sim.tune_teach(kernel=1)
    if side in QUEUED:
        sim.set_episode_queue(torch.as_tensor(queue))
        sim.begin_episodes(wrap=True)
    else:
        sim.reset(*specs)
    return sim


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
    for t in range(tick0 + 1, tick0 + steps + 1):
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
    ap.add_argument("--actions", default="hashed", choices=("hashed", "nostop"))
    ap.add_argument("--tree", default=None, help="checkout to import psketch_amd from (default: this one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    import psketch_amd as P
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs a GPU")
    sides = [s for s in a.sides.split(",") if s]
    if not set(sides) <= {"step", "stream", "lang", "lang_stream"}:
        raise SystemExit("--sides: step, stream, lang, lang_stream")
    n = a.envs
    lines = []
    for world, W in (("craft_medium_12x12", 12), ("craft_medium_12x12_w5", 12)):
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
        for teach in (False, True):
            bufs["labels"] = torch.empty(n, **i32) if teach else None
            us = {k: [] for k in sims}
            for r in range(a.runs + 1):          # run 0 warms every side and is dropped
                for k in sims:
                    v = timed(sims[k], a.steps, k, bufs, r * (a.steps + 1), specs)
                    if r:
                        us[k].append(round(v, 3))
            for s in sims.values():
                s.check()
            line = {"tree": tree, "world": world, "envs": n, "teacher": teach, "actions": a.actions, "steps": a.steps, "runs": a.runs,
                    "us_per_tick": us, "median_us": {k: statistics.median(v) for k, v in us.items()},
                    "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()}}
            med = line["median_us"]
            if set(us) == {"step", "stream"}:
                d = med["stream"] - med["step"]
                line["stream_minus_step_us"] = round(d, 3)
                line["within_spread"] = abs(d) <= max(line["spread_us"].values())
            elif len(us) > 1:
                for hi, lo in (("stream", "step"), ("lang_stream", "lang"), ("lang_stream", "stream")):
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
