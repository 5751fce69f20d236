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

    python tools/stream_bench.py [--envs 65536] [--steps 32] [--runs 9] [--sides step,stream]
                                 [--tree DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch


def make(P, world, n, pool, specs, queue, stream):
    sim = P.CraftSim(world, n_envs=n, device=0, pool_capacity=len(pool))
    sim.load_pool(pool)
    sim.tune_teach(kernel=1)
    if stream:
        sim.set_episode_queue(torch.as_tensor(queue))
        sim.begin_episodes(wrap=True)
    else:
        sim.reset(*specs)
    return sim


def timed(sim, steps, stream, bufs, tick0):
    kw = dict(obs=bufs["obs"], done=bufs["done"], labels=bufs["labels"])
    if stream:
        fn = sim.step_stream
        kw.update(episode_end=bufs["end"], end_pose=bufs["pose"], episode_now=bufs["now"])
    else:
        fn = sim.step
        kw["autoreset"] = True
    fn(None, seed=5, tick=tick0, **kw)                               # (warm)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(tick0 + 1, tick0 + steps + 1):
        fn(None, seed=5, tick=t, **kw)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--sides", default="step,stream")
    ap.add_argument("--tree", default=None, help="checkout to import psketch_amd from (default: this one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    import psketch_amd as P
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs a GPU")
    sides = [s for s in a.sides.split(",") if s]
    if not set(sides) <= {"step", "stream"}:
        raise SystemExit("--sides: step, stream")
    n = a.envs
    lines = []
    for world, W in (("craft_medium_12x12", 12), ("craft_medium_12x12_w5", 12)):
        probe = P.CraftSim(world, n_envs=64, device=0, pool_capacity=1)
        pool, _, _ = P.sample_scenarios(probe.params, probe.cookbook, 123, 256)
        tasks = [t.id for t in probe.task_manager.dataset_tasks()]
        queue = np.stack(P.synthetic_specs(pool, W, W, 2 * n + 17, 0, seed=0, task_ids=tasks), 1).astype(np.int32)
        specs = [torch.as_tensor(np.ascontiguousarray(queue[:n, j]), device="cuda") for j in range(5)]
        sims = {k: make(P, world, n, pool, specs, queue, k == "stream") for k in sides}
        i32 = dict(dtype=torch.int32, device="cuda")
        bufs = {"obs": next(iter(sims.values())).empty_obs(), "done": torch.empty(n, dtype=torch.uint8, device="cuda"),
                "end": torch.empty(n, **i32), "pose": torch.empty(n, **i32), "now": torch.empty(n, **i32)}
        for teach in (False, True):
            bufs["labels"] = torch.empty(n, **i32) if teach else None
            us = {k: [] for k in sims}
            for r in range(a.runs + 1):          # run 0 warms every side and is dropped
                for k in sims:
                    v = timed(sims[k], a.steps, k == "stream", bufs, r * (a.steps + 1))
                    if r:
                        us[k].append(round(v, 3))
            for s in sims.values():
                s.check()
            line = {"tree": tree, "world": world, "envs": n, "teacher": teach, "steps": a.steps, "runs": a.runs,
                    "us_per_tick": us, "median_us": {k: statistics.median(v) for k, v in us.items()},
                    "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()}}
            if len(us) == 2:
                d = line["median_us"]["stream"] - line["median_us"]["step"]
                line["stream_minus_step_us"] = round(d, 3)
                line["within_spread"] = abs(d) <= max(line["spread_us"].values())
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
