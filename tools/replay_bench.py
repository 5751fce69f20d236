#!/usr/bin/env python
"""craft_rollout_replay (the K-tick launch on the queue reading its actions from the installed
tape) against what it replaces, at 65,536 envs of 12x12 craft_medium.

`--mode kernel`: microseconds per tick of the launch alone, timed with device events around
`--launches` back-to-back launches of `--ticks` ticks into an observation ring of `--ring` slots,
wrap on, the sides alternating run by run:
  given      craft_rollout_stream fed the [ticks, n] action tensors computed on the host from the
             same tape (a fresh tensor per launch, resident before the timed window);
  tape       craft_rollout_replay, step_now / action_next NULL;
  tape_outs  craft_rollout_replay with both outputs set.
Every side takes the identical action stream: a seeded tape of one row per queue entry, lengths
3..24, each ending in its STOP.  The yardstick is `given` built from the PARENT commit: `--tree DIR`
imports the package (and its built library) from another checkout, which has the given side only,
so a caller alternates invocations of the two trees on one box.

`--mode pass`: wall-clock time of rollout.replay over a whole pass with a no-op on_chunk: 65,536
slots, a queue of 4 x 65,536 instances over a sampled pool (synthetic specs the
DemonstrationTeacher finishes, repeated to that number), the demonstrations rollout.demonstrations
records for them (a seeded tape of lengths 3..24 should that fail; the line says which), K = 32.  Beside the wall time the line carries the device-busy time: the sum
of device-event intervals around every launch of the pass (the K-tick launch and the summary).

    python tools/replay_bench.py --mode kernel [--sides given,tape,tape_outs] [--worlds w3,w5]
                                 [--envs 65536] [--ticks 20] [--launches 8] [--ring 16] [--runs 9]
                                 [--tree DIR] [--out FILE]
    python tools/replay_bench.py --mode pass [--envs 65536] [--factor 4] [--k 32] [--runs 3] [--padded]
                                 [--tree DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

STOP = 5
WORLDS = {"w3": ("craft_medium_12x12", 12), "w5": ("craft_medium_12x12_w5", 12)}


def seeded_tape(count, T, seed, lo=3, hi=24):
    """[count, T] int32, -1 padded: lengths lo..hi, actions 0..4, then the row's STOP."""
    rng = np.random.RandomState(seed)
    length = rng.randint(lo, min(hi, T) + 1, size=count)
    tape = rng.randint(0, 5, size=(count, T)).astype(np.int32)
    col = np.arange(T)[None]
    tape[col == length[:, None] - 1] = STOP
    tape[col >= length[:, None]] = -1
    return tape, length


def slot_streams(tape, length, n):
    """What the given side needs to lay out its tensors: per slot the cumulative lengths of its
    entries i, i + n, ... (the queue's length is a multiple of n, wrap on)."""
    m = len(tape) // n
    L = length.reshape(m, n)
    cum = np.concatenate([np.zeros((1, n), np.int64), np.cumsum(L, 0)])
    return cum, cum[-1]


def actions_of_ticks(tape, cum, period, n, t0, k):
    """[k, n] int32: slot i's action at ticks t0 .. t0 + k - 1 of its wrapped stream."""
    out = np.empty((k, n), dtype=np.int32)
    slots = np.arange(n)
    for j in range(k):
        r = (t0 + j) % period
        e = (r[None] >= cum[1:]).sum(0)
        out[j] = tape[slots + e * n, r - cum[e, slots]]
    return out


def kernel_mode(P, a, tree):
    n = a.envs
    sides = [s for s in a.sides.split(",") if s]
    lines = []
    for world, W in (WORLDS[w] for w in a.worlds.split(",") if w):
        probe = P.CraftSim(world, n_envs=64, device=0, pool_capacity=1)
        T = probe.config.max_timesteps
        pool, _, _ = P.sample_scenarios(probe.params, probe.cookbook, 123, 256)
        tasks = [t.id for t in probe.task_manager.dataset_tasks()]
        queue = np.stack(P.synthetic_specs(pool, W, W, 2 * n, 0, seed=0, task_ids=tasks), 1).astype(np.int32)
        tape, length = seeded_tape(len(queue), T, 7)
        cum, period = slot_streams(tape, length, n)
        per_run = (a.launches + 1) * a.ticks
        acts = None
        if "given" in sides:                             # every launch's tensor, resident up front
            acts = torch.as_tensor(actions_of_ticks(tape, cum, period, n, 0, (a.runs + 1) * per_run)).cuda()
        sims = {}
        for s in sides:
            sim = sims[s] = P.CraftSim(world, n_envs=n, device=0, pool_capacity=len(pool))
            sim.load_pool(pool)
            sim.set_episode_queue(torch.as_tensor(queue))
            if s != "given":
                sim.set_episode_actions(torch.as_tensor(tape))
            sim.begin_episodes(wrap=True)
        ring = torch.empty((a.ring, n, probe.n_features), dtype=sims[sides[0]].obs_dtype, device="cuda")
        outs = {k: torch.empty((a.ring, n), dtype=torch.int32, device="cuda") for k in ("step_now", "action_next")}

        def launch(s, t0):
            if s == "given":
                sims[s].rollout_stream(a.ticks, tick0=t0, actions=acts[t0:t0 + a.ticks], obs=ring)
            elif s == "tape":
                sims[s].rollout_replay(a.ticks, tick0=t0, obs=ring)
            else:
                sims[s].rollout_replay(a.ticks, tick0=t0, obs=ring, **outs)

        us = {s: [] for s in sides}
        for r in range(a.runs + 1):                      # run 0 warms every side and is dropped
            for s in sides:
                t0 = r * per_run
                launch(s, t0)                            # (warm)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for l in range(1, a.launches + 1):
                    launch(s, t0 + l * a.ticks)
                e1.record()
                e1.synchronize()
                if r:
                    us[s].append(round(e0.elapsed_time(e1) * 1e3 / (a.launches * a.ticks), 3))
        for sim in sims.values():
            sim.check()
        stats = {s: sims[s].stats().cpu().tolist() for s in sides}
        assert len({tuple(v) for v in stats.values()}) == 1, stats     # the sides ran the same episodes
        line = {"mode": "kernel", "tree": tree, "world": world, "envs": n, "ticks": a.ticks, "launches": a.launches,
                "ring": a.ring, "runs": a.runs, "us_per_tick": us,
                "median_us": {k: statistics.median(v) for k, v in us.items()},
                "range_us": {k: [min(v), max(v)] for k, v in us.items()}, "stats": stats[sides[0]]}
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def teachable(P, world, pool, specs, K):
    """The instances of `specs` rollout.demonstrations accepts (the teacher never raises, the
    episode ends in a STOP with its task satisfied): its pass (craft_rollout_teach_stream with
    label_actions, one craft_episode_summary per launch) on a handle of its own, keeping the
    results it would refuse.  Returns a bool mask."""
    n = min(65536, len(specs))
    sim = P.CraftSim(world, n_envs=n, device=0, pool_capacity=len(pool))
    sim.load_pool(pool)
    T = sim.config.max_timesteps
    sim.set_episode_queue(torch.as_tensor(specs))
    sim.begin_episodes()
    label_in, _ = sim.teacher()
    i32 = dict(dtype=torch.int32, device="cuda")
    labels, rec, ended, pose, now = (torch.empty((K, n), **i32) for _ in range(5))
    succ = torch.empty((K, n), dtype=torch.int8, device="cuda")
    run, summ = torch.zeros(n, **i32), {}
    raised = torch.zeros(len(specs) + 1, dtype=torch.bool, device="cuda")
    raised[:n] = label_in == -2
    for t0 in range(0, -(-len(specs) // n) * T, K):
        sim.rollout_teach_stream(K, tick0=t0, label_actions=True, label_in=label_in, labels=labels,
                                 action_record=rec, success=succ, episode_end=ended, end_pose=pose, episode_now=now)
        label_in = labels[K - 1].clone()
        raised[torch.where((labels == -2) & (now >= 0), now, len(specs)).reshape(-1).long()] = True
        summ = sim.episode_summary(ended, pose, succ, action_record=rec, count=len(specs), run=run,
                                   episode_now=now[K - 1], distances=False,
                                   **{k + "_out": v for k, v in summ.items() if v is not None})
        if bool((now[K - 1] < 0).all()):
            break
    try:
        sim.check()
    except Exception:                                    # the teacher's latched raise: those instances are dropped
        pass
    length, success, acts = (summ[k].cpu().numpy() for k in ("length", "success", "actions"))
    last = acts[np.arange(len(specs)), np.clip(length, 1, T) - 1]
    return (success == 1) & (length >= 1) & (length <= T) & (last == STOP) & ~raised[:-1].cpu().numpy()


def pass_mode(P, a, tree):
    from psketch_amd import rollout
    n, world, W = a.envs, *WORLDS["w3"]
    sim = P.CraftSim(world, n_envs=n, device=0, pool_capacity=256)
    T = sim.config.max_timesteps
    pool, _, _ = P.sample_scenarios(sim.params, sim.cookbook, 123, 256)
    sim.load_pool(pool)
    tasks = [t.id for t in sim.task_manager.dataset_tasks()]
    # candidates, of which the teacher finishes some: those, repeated in order up to factor * n
    cand = np.stack(P.synthetic_specs(pool, W, W, a.factor * n, 0, seed=0, task_ids=tasks), 1).astype(np.int32)
    keep = np.nonzero(teachable(P, world, pool, cand, a.k))[0]
    source = f"demonstrations ({len(keep)} of {len(cand)} candidates the teacher finishes, repeated)"
    try:
        specs = np.ascontiguousarray(cand[np.resize(keep, a.factor * n)])
        demo = rollout.demonstrations(sim, specs, ticks_per_launch=a.k)
        seqs = [row[:l] for row, l in zip(demo.action_seqs, demo.length)]
    except (rollout.RolloutError, ValueError) as e:
        specs = cand
        tape, length = seeded_tape(len(specs), T, 7)
        seqs, source = [row[:l] for row, l in zip(tape, length)], f"seeded tape ({e})"
    n_actions = int(sum(len(s) for s in seqs))
    if a.padded:                                         # the sequences as one [count, T] array, -1 padded
        arr = np.full((len(seqs), T), -1, dtype=np.int32)
        arr[np.arange(T)[None] < np.asarray([len(s) for s in seqs])[:, None]] = np.concatenate(seqs)
        seqs = arr
    busy = []
    for name in ("rollout_stream", "rollout_replay", "episode_summary"):
        inner = getattr(sim, name, None)
        if inner is None:
            continue

        def timed(*args, _inner=inner, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = _inner(*args, **kw)
            e1.record()
            busy.append((e0, e1))
            return out
        setattr(sim, name, timed)
    wall, dev, info = [], [], None
    for r in range(a.runs + 1):                          # run 0 warms and is dropped
        del busy[:]
        torch.cuda.synchronize()
        t = time.perf_counter()
        info = rollout.replay(sim, specs, seqs, ticks_per_launch=a.k, on_chunk=lambda *x: None)
        torch.cuda.synchronize()
        w = time.perf_counter() - t
        if r:
            wall.append(round(w * 1e3, 2))
            dev.append(round(sum(e0.elapsed_time(e1) for e0, e1 in busy), 2))
    line = {"mode": "pass", "tree": tree, "world": world, "envs": n, "instances": len(specs), "k": a.k,
            "sequences": source, "ticks": int(info.ticks), "launches": int(info.launches),
            "actions": n_actions, "input": "padded array" if a.padded else "list of arrays", "wall_ms": wall, "device_busy_ms": dev,
            "median_wall_ms": statistics.median(wall), "median_device_busy_ms": statistics.median(dev),
            "busy_share": round(statistics.median(dev) / statistics.median(wall), 4)}
    print(json.dumps(line), flush=True)
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="kernel", choices=("kernel", "pass"))
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--sides", default="given,tape,tape_outs")
    ap.add_argument("--worlds", default="w3,w5")
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--ring", type=int, default=16)
    ap.add_argument("--runs", type=int, default=None, help="timed runs per side (kernel: 9, pass: 3)")
    ap.add_argument("--factor", type=int, default=4, help="pass: instances per slot")
    ap.add_argument("--k", type=int, default=32, help="pass: ticks per launch")
    ap.add_argument("--padded", action="store_true",
                    help="pass: hand replay the sequences as one -1 padded array (this tree only)")
    ap.add_argument("--tree", default=None, help="checkout to import psketch_amd from (default: this one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs is None:
        a.runs = 9 if a.mode == "kernel" else 3
    tree = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    import psketch_amd as P
    if not torch.cuda.is_available():
        raise SystemExit("replay_bench needs a GPU")
    lines = kernel_mode(P, a, tree) if a.mode == "kernel" else pass_mode(P, a, tree)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
