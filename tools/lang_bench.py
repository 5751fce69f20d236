#!/usr/bin/env python
"""craft_step_lang (hashed actions, the teacher on) against the one-tile craft_step_teach
(tune_teach(kernel=1)): the same phases over the same bytes, plus one byte and one int8 per env.

Both on the same build and the same device, in alternating runs, at 65,536 envs of 12x12 worlds
with 3x3 and 5x5 windows, timed with device events around `--steps` back-to-back launches that
rewrite one observation buffer (a trainer's loop).  Episodes end and stay frozen under the
language protocol (it has no auto-reset), so both sides restart their envs before every timed
run and the timed window (default 32 ticks) stays inside max_timesteps = 40: every env steps in
every timed tick on both sides, except the few the hashed policy STOPs.

Prints one JSON line per window: the per-run microseconds per tick of both, their medians and
the spread of the alternating runs (max - min of each side's runs); `within_spread` says whether
the medians differ by no more than the larger spread.

    python tools/lang_bench.py [--envs 65536] [--steps 32] [--runs 9] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from psketch_amd import CraftSim, sample_scenarios, synthetic_specs  # noqa: E402


def make(world, n, pool, specs):
    sim = CraftSim(world, n_envs=n, device=0, pool_capacity=len(pool))
    sim.load_pool(pool)
    sim.tune_teach(kernel=1)
    sim.reset(*specs)
    return sim


def timed(sim, specs, steps, lang, bufs):
    obs, done, labels = bufs
    sim.reset(*specs)
    fn = sim.step_lang if lang else sim.step
    kw = {} if lang else {"autoreset": False}
    fn(None, seed=5, tick=0, obs=obs, done=done, labels=labels, **kw)      # (tick 0: warm)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(1, steps + 1):
        fn(None, seed=5, tick=t, obs=obs, done=done, labels=labels, **kw)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lang_bench needs a GPU")
    lines = []
    for world, W in (("craft_medium_12x12", 12), ("craft_medium_12x12_w5", 12)):
        probe = CraftSim(world, n_envs=64, device=0, pool_capacity=1)
        if a.steps + 1 >= probe.config.max_timesteps:
            raise SystemExit("--steps must stay inside max_timesteps")
        pool, _, _ = sample_scenarios(probe.params, probe.cookbook, 123, 256)
        tasks = [t.id for t in probe.task_manager.dataset_tasks()]
        specs = [torch.as_tensor(s, device="cuda") for s in
                 synthetic_specs(pool, W, W, a.envs, 0, seed=0, task_ids=tasks)]
        sims = {"step_teach": make(world, a.envs, pool, specs), "step_lang": make(world, a.envs, pool, specs)}
        bufs = (sims["step_lang"].empty_obs(), torch.empty(a.envs, dtype=torch.uint8, device="cuda"),
                torch.empty(a.envs, dtype=torch.int32, device="cuda"))
        us = {k: [] for k in sims}
        for r in range(a.runs + 1):              # run 0 warms both and is dropped
            for k in sims:
                v = timed(sims[k], specs, a.steps, k == "step_lang", bufs)
                if r:
                    us[k].append(round(v, 3))
        for s in sims.values():
            s.check()
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: round(max(v) - min(v), 3) for k, v in us.items()}
        kname, envs, lanes = sims["step_teach"].step_shape(teach=True)
        line = {"world": world, "envs": a.envs, "steps": a.steps, "runs": a.runs,
                "kernel": kname, "tile_envs": envs, "teacher_lanes": lanes,
                "us_per_tick": us, "median_us": med, "spread_us": spread,
                "lang_minus_teach_us": round(med["step_lang"] - med["step_teach"], 3),
                "within_spread": abs(med["step_lang"] - med["step_teach"]) <= max(spread.values())}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
