"""Where the trainer loop's per-tick time goes (bench.py --workload trainer): device time per
tick of back-to-back sequences queued without any host wait, so that only the kernels and the
gaps between them count:

  policy   the stand-in student alone (addmm + argmax + int32 cast), 40 ticks
  step     craft_step_teach alone (student actions precomputed), 40 ticks
  step_plain / teacher   craft_step_ex and craft_teacher alone
  both     policy then step per tick, 40 ticks (one do_rollout's device work)
  side_teacher   craft_teacher on a side stream beside the policy, then craft_step_ex
  graph    `both` captured as one HIP graph and replayed
  head_argmax   addmm, then craft_step_policy (the tick chooses the first maximum itself) with the
                teacher: `both` without the argmax and cast kernels and their [n] round trip
  torch_sample  addmm + Categorical(logits).sample() + cast + craft_step_teach: the training loop
  head_sample   addmm, then craft_step_policy drawing from the softmax in the tick
  head_split    addmm, craft_policy_actions, craft_step_teach: the head as a launch of its own
                (each of the four also as a graph: <name>_graph)

    python tools/loop_probe.py [--envs 65536] [--reps 5]

--lang: the language trainers' loop instead, on craft_step_lang_stream with wrap (no slot ever
freezes, so every tick does the same work), the sequences of a repetition run in turn (parent
path, head path, ...: the alternation the comparison needs):

  lang_eval_torch     addmm + argmax + cast + craft_step_lang_stream: evaluate() as it was
  lang_eval_head      addmm, then craft_step_lang_policy_stream (argmax in the tick)
  lang_active_torch   the active training tick as it was: addmm, Categorical(logits): sample + cast,
                      entropy / log(6) > threshold + cast; the instructed addmm, Categorical.sample +
                      cast; craft_step_lang_stream with the teacher (alt_actions, use_alt)
  lang_active_head    addmm, craft_policy_ask, the instructed addmm, craft_step_lang_policy_stream with
                      both heads sampling and the teacher
  lang_active_split   addmm, craft_policy_ask, the instructed addmm, craft_policy_actions twice, then
                      craft_step_lang_stream: the heads as launches of their own
  lang_tick / lang_tick_head / lang_tick_2heads   the tick alone on fixed inputs, teacher on: integer
                      actions + alt_actions; one head; both heads (sample).  lang_kernels_us: the
                      tile kernel's mean duration in each of the three, from the profiler

    python tools/loop_probe.py --lang [--envs 65536] [--reps 5] [--threshold 0.5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from psketch_amd import CraftSim, sample_scenarios, synthetic_specs  # noqa: E402


def lang_main(args):
    import math
    n, T, thr = args.envs, 40, args.threshold
    sim = CraftSim("craft_medium_12x12", n_envs=n, device=0, pool_capacity=1024)
    grids, _, _ = sample_scenarios(sim.params, sim.cookbook, 123, 1024)
    sim.load_pool(grids)
    tasks = [t.id for t in sim.task_manager.dataset_tasks()]
    specs = torch.stack([torch.as_tensor(s) for s in synthetic_specs(grids, 12, 12, 2 * n + 17, 0, seed=0,
                                                                    task_ids=tasks)], 1).to(torch.int32)
    _, W, bias = bench.trainer_policy(sim.n_features, sim.device)
    Wd = torch.as_tensor(W, dtype=torch.float32, device=sim.device)
    bd = torch.as_tensor(bias, dtype=torch.float32, device=sim.device)
    dev = sim.device
    obs = sim.empty_obs()
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    ask8 = torch.empty(n, dtype=torch.uint8, device=dev)
    a1, a2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    cat = lambda L: torch.distributions.Categorical(logits=L, validate_args=False)   # noqa: E731

    def main_logits(t, alpha):                            # the main model up to its last GEMM
        return torch.addmm(bd, obs, Wd[t % Wd.shape[0]], alpha=alpha)

    def instructed_logits(t):                             # the instructed model's (other weights)
        return torch.addmm(bd, obs, Wd[(t + 1) % Wd.shape[0]], alpha=0.25)

    def eval_torch(t):
        sim.step_lang_stream(main_logits(t, 8).argmax(dim=1).to(torch.int32), tick=t, obs=obs)

    def eval_head(t):
        sim.step_lang_stream(logits=main_logits(t, 8), head="argmax", tick=t, obs=obs)

    def active_torch(t):
        d = cat(main_logits(t, 0.25))
        a = d.sample().to(torch.int32)
        ask = (d.entropy() / math.log(6) > thr).to(torch.uint8)
        alt = cat(instructed_logits(t)).sample().to(torch.int32)
        sim.step_lang_stream(a, tick=t, alt_actions=alt, use_alt=ask, obs=obs, labels=labels)

    def active_head(t):
        L = main_logits(t, 0.25)
        sim.policy_ask(L, thr, out=ask8)
        sim.step_lang_stream(logits=L, head="sample", head_seed=11, alt_logits=instructed_logits(t), alt_head="sample",
                             alt_head_seed=10, use_alt=ask8, tick=t, obs=obs, labels=labels)

    def active_split(t):
        L = main_logits(t, 0.25)
        sim.policy_ask(L, thr, out=ask8)
        sim.policy_actions(L, "sample", seed=11, tick=t, out=a1)
        sim.policy_actions(instructed_logits(t), "sample", seed=10, tick=t, out=a2)
        sim.step_lang_stream(a1, tick=t, alt_actions=a2, use_alt=ask8, obs=obs, labels=labels)

    fixed_L = torch.randn(n, 6, device=dev)
    fixed_A = torch.randn(n, 6, device=dev)
    fixed_a = torch.randint(0, 5, (n,), dtype=torch.int32, device=dev)
    fixed_alt = torch.randint(0, 5, (n,), dtype=torch.int32, device=dev)
    fixed_ask = (torch.arange(n, device=dev) % 3 == 0).to(torch.uint8)

    def tick(t):
        sim.step_lang_stream(fixed_a, tick=t, alt_actions=fixed_alt, use_alt=fixed_ask, obs=obs, labels=labels)

    def tick_head(t):
        sim.step_lang_stream(logits=fixed_L, head="sample", head_seed=11, tick=t, alt_actions=fixed_alt,
                             use_alt=fixed_ask, obs=obs, labels=labels)

    def tick_2heads(t):
        sim.step_lang_stream(logits=fixed_L, head="sample", head_seed=11, alt_logits=fixed_A, alt_head="sample",
                             alt_head_seed=10, use_alt=fixed_ask, tick=t, obs=obs, labels=labels)

    ticks = {"lang_eval_torch": eval_torch, "lang_eval_head": eval_head, "lang_active_torch": active_torch,
             "lang_active_head": active_head, "lang_active_split": active_split, "lang_tick": tick,
             "lang_tick_head": tick_head, "lang_tick_2heads": tick_2heads}
    sim.set_episode_queue(specs)
    sim.begin_episodes(wrap=True, obs=obs)
    for f in ticks.values():                              # warm every shape
        for t in range(T):
            f(t)
    sim.sync_table()
    us = {name: [] for name in ticks}
    for _ in range(args.reps):                            # the sequences in turn, every repetition
        for name, f in ticks.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in range(T):
                f(t)
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / T)
    out = {"envs": n, "ticks": T, "threshold": thr, "reps": args.reps}
    for name, v in us.items():
        out[name + "_us_per_tick"] = round(min(v), 2)
        out[name + "_us_per_tick_all"] = [round(x, 2) for x in v]
    out["lang_kernels_us"] = {name: bench.profiled_kernel_us(lambda f=f: f(0), 16, "tile_kernel")
                              for name, f in (("lang_tick", tick), ("lang_tick_head", tick_head),
                                              ("lang_tick_2heads", tick_2heads))}
    out["ask_rate"] = round(float(ask8.float().mean()), 3)
    sim.check()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lang", action="store_true", help="the language trainers' loop (see above)")
    ap.add_argument("--threshold", type=float, default=0.5, help="--lang: the active student's ask threshold")
    args = ap.parse_args()
    if args.lang:
        return lang_main(args)
    n, T = args.envs, 40
    sim = CraftSim("craft_medium_12x12", n_envs=n, device=0, pool_capacity=1024)
    grids, _, _ = sample_scenarios(sim.params, sim.cookbook, 123, 1024)
    sim.load_pool(grids)
    tasks = [t.id for t in sim.task_manager.dataset_tasks()]
    specs = synthetic_specs(grids, 12, 12, n, 0, seed=0, task_ids=tasks)
    act, W, bias = bench.trainer_policy(sim.n_features, sim.device)
    Wd = torch.as_tensor(W, dtype=torch.float32, device=sim.device)
    bd = torch.as_tensor(bias, dtype=torch.float32, device=sim.device)
    head_acts = torch.empty(n, dtype=torch.int32, device=sim.device)

    def logits(t):                                        # the student up to its last GEMM
        return torch.addmm(bd, obs, Wd[t % Wd.shape[0]], alpha=8)

    def head_tick(t, mode):
        sim.step(logits=logits(t), head=mode, head_seed=11, tick=t, autoreset=True, obs=obs, labels=labels[t + 1])

    def torch_sample_tick(t):
        a = torch.distributions.Categorical(logits=logits(t), validate_args=False).sample().to(torch.int32)
        sim.step(a, tick=t, autoreset=True, obs=obs, labels=labels[t + 1])

    def head_split_tick(t):
        sim.policy_actions(logits(t), "argmax", tick=t, out=head_acts)
        sim.step(head_acts, tick=t, autoreset=True, obs=obs, labels=labels[t + 1])
    obs = sim.empty_obs()
    labels = torch.empty((T + 1, n), dtype=torch.int32, device=sim.device)
    acts = torch.randint(0, 5, (n,), dtype=torch.int32, device=sim.device)

    def policy(t):
        return act(obs, t)

    def step(t, a):
        sim.step(a, tick=t, autoreset=True, obs=obs, labels=labels[t + 1])

    side = torch.cuda.Stream()
    main = torch.cuda.current_stream()
    ev = [torch.cuda.Event() for _ in range(T)]

    def step_plain(t, a):
        sim.step(a, tick=t, autoreset=True, obs=obs)

    def side_tick(t):
        # the teacher's labels of the current states on a side stream, beside the student
        side.wait_stream(main)
        with torch.cuda.stream(side):
            sim.teacher(action_out=labels[t])
        ev[t].record(side)
        a = policy(t)
        main.wait_event(ev[t])
        step_plain(t, a)

    seqs = {
        "policy": lambda: [policy(t) for t in range(T)],
        "step": lambda: [step(t, acts) for t in range(T)],
        "step_plain": lambda: [step_plain(t, acts) for t in range(T)],
        "teacher": lambda: [sim.teacher(action_out=labels[t]) for t in range(T)],
        "both": lambda: [step(t, policy(t)) for t in range(T)],
        "side_teacher": lambda: [side_tick(t) for t in range(T)],
        "head_argmax": lambda: [head_tick(t, "argmax") for t in range(T)],
        "torch_sample": lambda: [torch_sample_tick(t) for t in range(T)],
        "head_sample": lambda: [head_tick(t, "sample") for t in range(T)],
        "head_split": lambda: [head_split_tick(t) for t in range(T)],
    }
    sim.reset(*specs)
    for f in seqs.values():
        f()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        seqs["both"]()
    seqs["graph"] = g.replay
    for name in ("head_argmax", "torch_sample", "head_sample", "head_split"):
        gh = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(gh):
            seqs[name]()
        seqs[name + "_graph"] = gh.replay
    out = {"envs": n, "ticks": T}
    for name, f in seqs.items():
        us = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / T)
        out[name + "_us_per_tick"] = round(min(us), 2)
    out["policy_kernels_us"] = bench.profiled_kernel_us(lambda: policy(0), 8, "Cijk")
    sim.check()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
