"""Batched ImitationTrainer.do_rollout on the GPU (trainers/imitation.py:18-101).

The reference rolls a batch out one env at a time in Python: per tick,
student.act(states) over stacked features(), the DemonstrationTeacher for each
live env, the behaviour-cloning substitution, the timer/STOP protocol, step.
Here the whole batch lives in CraftSim slots and every per-env part of a tick is
a kernel on the current stream:

  craft_teacher           ref_actions, -1 for done (frozen) envs      (imitation.py:47-55)
  craft_step_ex           bc ? ref : student (imitation.py:56-57), action_seqs row
                          (:59-61), timer/STOP/satisfies/step + features (:63-73),
                          and an any-env-still-running flag (:42)

The student sees the features as a device tensor and returns device actions;
nothing crosses PCIe inside the loop except the all(done) test (imitation.py:42):
the step kernels store each tick's any-live flag straight into page-locked host
memory, which the host reads once the tick's event has completed.  After the loop, one
launch (craft_rollout_distances) computes every env's `distances` entry (imitation.py:79-91:
failed get tasks search their initial grid from their final pose with
find_closest_resources' BFS), is_get and action count, and the summary comes back in one
transfer.
"""
import ctypes
import gc
import inspect
import time
import weakref

import numpy as np
import torch

from . import _native as N
from .sim import CraftSim, _stack_specs


class RolloutError(Exception):
    """Raised where the reference's do_rollout raises (TypeError/AssertionError)."""


class _Info:
    """A driver's results: the fields its class documents, as attributes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class RolloutInfo(_Info):
    """do_rollout's `info` as device tensors.

    action_seqs int32 [T, n] (-1 after an env's last action), n_actions int32 [n],
    success int8 [n], distances int32 [n] (-1 where the task is not a get task),
    is_get bool [n], num_interactions / num_steps ints, ticks, and obs
    ([T+1, n, F], every observation the student saw) when kept."""

    def to_reference(self):
        """The reference's info dict (python lists, trainers/imitation.py:93-99)."""
        A = self.action_seqs.t().cpu().numpy()
        L = self.n_actions.cpu().numpy()
        succ = self.success.cpu().numpy()
        dist = self.distances.cpu().numpy()
        is_get = self.is_get.cpu().numpy()
        return {
            "action_seqs": [[int(a) for a in A[i, :L[i]]] for i in range(len(L))],
            "success": [bool(s) for s in succ],
            "distances": [int(d) for d, g in zip(dist, is_get) if g],
            "num_interactions": int(self.num_interactions),
            "num_steps": int(self.num_steps),
        }


def do_rollout(sim, spec, act, is_eval, behavior_clone=None, receive=None, keep_obs=False,
               timing=None, fused_teacher=True, lookahead=False, graph=0, graph_key=None, head=None,
               head_seed=0):
    """One rollout of sim.n_envs episodes.

    spec: (scenario, x, y, dir, task), each n_envs ints (device or host).
    act(obs, t) -> int device tensor [n]: the student (students/imitation.py act);
      obs is [n, F] on the device in the simulator's obs format (fp32 unless
      sim.set_obs_format) and is overwritten by the next step unless keep_obs.
    behavior_clone: [n] 0/1 (config.random.binomial(1, policy_mix_rate, n),
      imitation.py:39-41); ignored when is_eval.
    receive(ref_actions) is called once per tick when not is_eval
      (student.receive, imitation.py:75-77) with the int32 device tensor.
    timing: optional dict; receives host wall seconds of the setup, the tick
      loop and the distances/summary phases (each ends at a device sync).
    fused_teacher: when not is_eval, each tick's step also labels the new states
      (craft_step_teach: the next tick's ref_actions, in the same launch);
      False runs craft_teacher on a side stream, overlapping the student (with graph=G the
      fork and join are captured in the graphs: the teacher of tick t's states beside act(t),
      then craft_step_ex).
    lookahead: the all(done) test of tick t (imitation.py:42) no longer blocks the
      host before tick t + 1 is queued: tick t + 1 (act and step) is queued behind tick
      t's event, and only then is tick t's any-live flag read.  When tick t ended every episode the queued tick is discarded: its step
      is a no-op on frozen envs (no state, counter, success or action-record change that
      the result keeps), but act was called once more than the reference calls it, so
      lookahead is for side-effect-free students (a fixed or deterministic policy);
      receive() is still called exactly once per real tick.  Needs is_eval or the fused
      teacher.
    graph: G > 0 runs the ticks as HIP graphs of G ticks each (act + step per tick, captured
      with torch.cuda.graph on the first call for this simulator and this `act`, replayed by
      later calls), so the per-tick host work (the student's launches, the step's ctypes call)
      leaves the loop.  The conditions of lookahead apply, and more: act only queues device work
      on the current stream, with fixed shapes and no host synchronisation, and its device
      inputs stay where they were at capture (weights may change in place).  Chunk c + 1 is
      queued before chunk c's flags are read; ticks after the one that ended every episode are
      no-ops and are discarded.  The rollout's buffers are the simulator's own: the results are
      copies, and receive() is called once per real tick after the loop, in tick order, with
      rows of a copy of the labels.  Not with keep_obs.
    head: None, "argmax" or "sample".  With a head, act(obs, t) returns the student's float32
      [n, 6] logits instead of actions and the tick chooses each env's action itself
      (craft_step_policy: the first maximum, or a draw from the softmax keyed by head_seed, the
      env's global id and t), so no argmax / Categorical.sample kernels and no [n] round trip run
      between the student's last GEMM and the step.  Works with graph and lookahead alike.
    graph_key: a hashable naming what the captured graphs read besides the simulator (the
      student's state); the graphs are reused only while act is the same callable and the key is
      equal, and captured anew otherwise.  A student that re-allocates a tensor act reads (a
      new weight tensor instead of an in-place update) must change the key, e.g.
      tuple(p.data_ptr() for p in model.parameters()), or call drop_graphs(sim): a replay would
      read the old allocation.
    """
    if graph:
        return _graph_rollout(sim, spec, act, is_eval, behavior_clone, receive, keep_obs, timing,
                              fused_teacher, int(graph), graph_key, head, head_seed)
    t_start = time.perf_counter()
    n, dev, T = sim.n_envs, sim.device, sim.config.max_timesteps
    if T <= 0:
        raise ValueError("max_timesteps must be positive")
    spec = [sim._i32(a, n) for a in spec]
    task = spec[4]
    obs_hist = (torch.empty((T + 1, n, sim.n_features), dtype=sim.obs_dtype, device=dev)
                if keep_obs else None)
    obs = obs_hist[0] if keep_obs else sim.empty_obs()
    sim.reset(*spec, obs=obs)
    success = torch.zeros(n, dtype=torch.int8, device=dev)
    seqs = torch.full((T, n), -1, dtype=torch.int32, device=dev)
    live = _LiveFlags(sim, T)
    # ref_actions of every tick: tick t reads refs[t] and (fused) labels refs[t + 1]; receive()
    # gets the row itself (no copy), which no later tick or rollout overwrites
    refs = None if is_eval else torch.empty((T + 1, n), dtype=torch.int32, device=dev)
    bc = None if is_eval else _bc_mask(behavior_clone, n, dev)
    fused = not is_eval and fused_teacher
    if lookahead and not is_eval and not fused_teacher:
        raise ValueError("lookahead needs is_eval or fused_teacher")
    # The teacher reads only the env states, so without the fused teacher tick t's labels are
    # computed on a side stream while the student's act(t) runs on the main stream.
    # (the CPU variant, CraftSim(device="cpu"), runs every call synchronously: no streams)
    main = None if sim._cpu else torch.cuda.current_stream(dev)
    side = None
    if not is_eval and not fused_teacher:
        if sim._cpu:
            raise ValueError("the CPU variant runs the fused teacher only (fused_teacher=True)")
        side = _teacher_stream(sim)
    labels_ready = getattr(sim, "_teacher_event", None)
    if labels_ready is None and not sim._cpu:
        labels_ready = sim._teacher_event = torch.cuda.Event()

    def launch_teacher(t):
        side.wait_stream(main)                   # after the previous step
        with torch.cuda.stream(side):
            sim.teacher(action_out=refs[t])      # done (frozen) envs get -1
        labels_ready.record(side)

    step = _stepper(sim, fused, bc, success, head, head_seed)
    cur = {"obs": obs}

    def issue(t):
        """Tick t on the stream: the student's act, then one step launch (behaviour cloning, the
        action record, the any-live flag and, fused, the next tick's labels), then the flag's
        event (after the flag's copy to the host where it is not mapped)."""
        actions = _policy_output(act(cur["obs"], t), n, dev, head)
        if side is not None:
            main.wait_event(labels_ready)
        if keep_obs:
            cur["obs"] = obs_hist[t + 1]
        step(t, actions, cur["obs"], None if is_eval else refs[t], seqs[t], live.ptr(t),
             refs[t + 1] if fused else None)
        if side is not None and t + 1 < T:
            launch_teacher(t + 1)                # speculative: all -1 if every env is done
        live.record(t)

    if not is_eval:
        if fused_teacher:
            sim.teacher(action_out=refs[0])      # the initial states' labels; then every step's
        else:
            launch_teacher(0)
    t_loop = time.perf_counter()
    # every env is done once its timer reaches 0 (imitation.py:42, 62-63): tick t's flag is read
    # after its event; with lookahead, tick t + 1 is queued first (and discarded if every
    # episode ended at tick t)
    issue(0)
    t = 0
    while True:
        if lookahead and t + 1 < T:
            issue(t + 1)
        more = live.wait(t)
        if not is_eval and receive is not None:
            receive(refs[t])                     # tick t is real
        t += 1
        if t >= T or not more:
            break
        if not lookahead:
            issue(t)
    if side is not None:
        main.wait_stream(side)
    t_end_loop = time.perf_counter()
    return _finish(sim, task, success, seqs, t, is_eval, keep_obs, obs_hist, timing, t_start,
                   t_loop, t_end_loop, dev)


def _stepper(sim, teach, bc, success, head=None, head_seed=0):
    """do_rollout's per-tick craft_step_ex / craft_step_teach (include/craft.h) with the argument
    struct built once: a tick sets only its pointers and the tick number (every buffer is one
    do_rollout allocated and shaped itself, or the student's int32 [n] actions).  With a head the
    student's output is its float32 [n, 6] logits and the call is craft_step_policy."""
    if head is not None:
        return _policy_stepper(sim, teach, bc, success, head, head_seed)
    args = N.craft_step_args_t()
    args.flags = 0                                         # no auto-reset: done envs freeze
    if bc is not None:
        args.behavior_clone = bc.data_ptr()
    args.success = success.data_ptr()
    lib = sim._L
    fn = lib.craft_step_teach if teach else lib.craft_step_ex
    h, pargs, di = sim._h, ctypes.byref(args), sim.device.index
    raw = (lambda _: None) if sim._cpu else torch._C._cuda_getCurrentRawStream

    def step(t, actions, obs, ref, rec, live_ptr, labels):
        args.actions = actions.data_ptr()
        args.tick = t
        args.obs = obs.data_ptr()
        args.ref_actions = None if ref is None else ref.data_ptr()
        args.action_record = rec.data_ptr()
        args.any_live = live_ptr
        st = fn(h, pargs, labels.data_ptr(), raw(di)) if teach else fn(h, pargs, raw(di))
        if st:
            N.check(st, h, "craft_step_teach" if teach else "craft_step_ex", L=lib)
    return step


def _head_struct(head, head_seed):
    if head not in N.HEAD_MODES:
        raise ValueError(f"head must be None, 'argmax' or 'sample', got {head!r}")
    hd = N.craft_policy_head_t()
    hd.mode = N.HEAD_MODES[head]
    hd.seed = int(head_seed) & (2**64 - 1)
    return hd


def _policy_stepper(sim, teach, bc, success, head, head_seed):
    """_stepper's twin for do_rollout(head=...): craft_step_policy, label_out set when `teach`."""
    args = N.craft_step_args_t()
    args.flags = 0
    if bc is not None:
        args.behavior_clone = bc.data_ptr()
    args.success = success.data_ptr()
    hd = _head_struct(head, head_seed)
    lib = sim._L
    fn = lib.craft_step_policy
    h, pargs, phead, di = sim._h, ctypes.byref(args), ctypes.byref(hd), sim.device.index
    raw = (lambda _: None) if sim._cpu else torch._C._cuda_getCurrentRawStream

    def step(t, logits, obs, ref, rec, live_ptr, labels):
        hd.logits = logits.data_ptr()
        args.tick = t
        args.obs = obs.data_ptr()
        args.ref_actions = None if ref is None else ref.data_ptr()
        args.action_record = rec.data_ptr()
        args.any_live = live_ptr
        st = fn(h, pargs, phead, labels.data_ptr() if teach else None, raw(di))
        if st:
            N.check(st, h, "craft_step_policy", L=lib)
    return step


def _bc_mask(behavior_clone, n, dev):
    if behavior_clone is None:
        raise ValueError("behavior_clone is required when not is_eval")
    bc = torch.as_tensor(np.asarray(behavior_clone) if not torch.is_tensor(behavior_clone)
                         else behavior_clone, device=dev)
    if bc.numel() != n:
        raise ValueError(f"behavior_clone has {bc.numel()} entries, expected {n}")
    return (bc.reshape(n) != 0).to(torch.uint8).contiguous()


def drop_graphs(sim):
    """Forget the HIP graphs do_rollout(graph=G) captured for `sim` (the next graph rollout
    captures again): after the student re-allocated a tensor its act reads."""
    sim._graph_state = None


def _graph_rollout(sim, spec, act, is_eval, behavior_clone, receive, keep_obs, timing,
                   fused_teacher, G, graph_key=None, head=None, head_seed=0):
    """do_rollout(graph=G): see do_rollout."""
    t_start = time.perf_counter()
    n, dev, T = sim.n_envs, sim.device, sim.config.max_timesteps
    if keep_obs:
        raise ValueError("graph mode does not keep observations (keep_obs)")
    if G < 1:
        raise ValueError("graph: ticks per graph must be positive")
    if T <= 0:
        raise ValueError("max_timesteps must be positive")
    spec = [sim._i32(a, n) for a in spec]
    task = spec[4]
    live = _LiveFlags(sim, T)
    if not live.dev:
        raise RuntimeError("graph mode needs the any-live flags in mapped host memory")
    flags, events = live.host, live.events       # one event per chunk, read flag by flag
    gs = getattr(sim, "_graph_state", None)
    side_teacher = not is_eval and not fused_teacher
    key = (is_eval, G, T, graph_key, side_teacher, head, head_seed)
    if gs is None or not _same_act(gs["act"], act) or gs["key"] != key:
        sim._graph_state = None                  # drop the old graphs before capturing new ones
        gs = sim._graph_state = {
            "act": _weak_act(act), "key": key, "graphs": [],
            "obs": sim.empty_obs(), "success": torch.zeros(n, dtype=torch.int8, device=dev),
            "seqs": torch.full((T, n), -1, dtype=torch.int32, device=dev),
            "refs": None if is_eval else torch.empty((T + 1, n), dtype=torch.int32, device=dev),
            "bc": None if is_eval else torch.zeros(n, dtype=torch.uint8, device=dev)}
    obs, success, seqs, refs = gs["obs"], gs["success"], gs["seqs"], gs["refs"]
    sim.reset(*spec, obs=obs)
    success.zero_()
    # (every tick writes its whole action-record row; rows past the last tick are filled after
    # the loop, usually none)
    if not is_eval:
        gs["bc"].copy_(_bc_mask(behavior_clone, n, dev))
        sim.teacher(action_out=refs[0])          # the initial states' labels; then every step's
    nch = (T + G - 1) // G
    if not gs["graphs"]:
        step = _stepper(sim, not is_eval and not side_teacher, gs["bc"], success, head, head_seed)
        main = torch.cuda.current_stream(dev)
        side = _teacher_stream(sim) if side_teacher else None

        def issue(t):
            # (side teacher) tick t's ref_actions, the labels of the states tick t - 1 left, on a
            # forked stream beside the student's act(t); the step joins it (tick 0's come from
            # the eager call before the loop)
            cur = torch.cuda.current_stream(dev)    # (the capture's stream)
            if side is not None and t > 0:
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    sim.teacher(action_out=refs[t])
            actions = _policy_output(act(obs, t), n, dev, head)
            if side is not None and t > 0:
                cur.wait_stream(side)
            step(t, actions, obs, None if is_eval else refs[t], seqs[t], live.ptr(t),
                 None if is_eval or side is not None else refs[t + 1])

        warm = torch.cuda.Stream(dev)            # the student's libraries warmed off the capture
        warm.wait_stream(main)
        with torch.cuda.stream(warm):
            act(obs, 0)
        main.wait_stream(warm)
        pool = None
        graphs = []                              # cached only once every chunk is captured
        try:
            for c in range(nch):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool):
                    for t in range(c * G, min(T, (c + 1) * G)):
                        issue(t)
                pool = g.pool()
                graphs.append(g)
        except BaseException:
            sim._graph_state = None              # a failed capture leaves nothing behind
            raise
        gs["graphs"] = graphs
    graphs = gs["graphs"]
    t_loop = time.perf_counter()
    graphs[0].replay()
    events[0].record()
    ticks = None
    c = 0
    while ticks is None:
        if c + 1 < nch:                          # queued before chunk c's flags are read
            graphs[c + 1].replay()
            events[c + 1].record()
        events[c].synchronize()
        for t in range(c * G, min(T, (c + 1) * G)):
            if int(flags[t]) == 0:               # every episode ended at tick t (imitation.py:42)
                ticks = t + 1
                break
        c += 1
        if ticks is None and c >= nch:
            ticks = T
    if ticks < T:
        seqs[ticks:].fill_(-1)
    if not is_eval and receive is not None:
        labels = refs[:ticks].clone()
        for t in range(ticks):
            receive(labels[t])
    t_end_loop = time.perf_counter()
    return _finish(sim, task, success.clone(), seqs.clone(), ticks, is_eval, False, None, timing,
                   t_start, t_loop, t_end_loop, dev)


def _weak_act(act):
    """A weak reference to the student's act for the graph cache, so the cache does not keep the
    model alive (WeakMethod for a bound method: `student.act` is a new object on every access;
    a plain strong reference for callables that take no weak references)."""
    try:
        return weakref.WeakMethod(act) if inspect.ismethod(act) else weakref.ref(act)
    except TypeError:
        return lambda: act


def _same_act(ref, act):
    """Whether the cached graphs were captured for this act: equality, which bound methods
    define as the same function on the same object."""
    cached = ref()
    return cached is not None and cached == act


def _actions(a, n, dev):
    """The student's actions as an int32 [n] device tensor (one that already is: itself, no
    device work)."""
    if not torch.is_tensor(a):
        a = torch.as_tensor(np.asarray(a), device=dev)
    return a.to(device=dev, dtype=torch.int32).reshape(n).contiguous()


def _policy_output(a, n, dev, head):
    """What the student's act returned, as the step takes it: int32 [n] actions, or with a head
    its float32 [n, 6] logits (a tensor on the simulator's device; made contiguous float32)."""
    if head is None:
        return _actions(a, n, dev)
    if not torch.is_tensor(a) or a.device != dev or tuple(a.shape) != (n, N.N_ACTIONS):
        raise ValueError(f"with head={head!r} act must return a [{n}, {N.N_ACTIONS}] logits tensor on {dev}")
    return a.to(torch.float32).contiguous()


def _teacher_stream(sim):
    """The side stream the unfused teacher runs on, created once per simulator (costly)."""
    side = getattr(sim, "_teacher_stream", None)
    if side is None:
        side = sim._teacher_stream = torch.cuda.Stream(sim.device)
    return side


class _LiveFlags:
    """The any-live flags of a driver's ticks (1: some env still running after tick t), one per
    tick: a page-locked host int32 array (`host`; zeroed here, reused across rollouts: the
    previous rollout's ticks have completed when it returned) that the kernel stores into
    directly where HIP maps it (`dev`, its device address from craft_host_flag_pointer), else
    (`dev` 0) a device array copied back per tick; and one event per tick (`events`).  The three
    are cached on the simulator as _live_host, _live_dev and _live_events."""

    def __init__(self, sim, T):
        flags = getattr(sim, "_live_host", None)
        if sim._cpu and (flags is None or flags.numel() < T + 1):
            # the CPU variant's "device" memory is the host's, and its calls have completed on return
            flags = sim._live_host = torch.zeros(max(T + 1, 64), dtype=torch.int32)
            sim._live_events = [_NoEvent()] * flags.numel()
            sim._live_dev = flags.data_ptr()
        elif flags is None or flags.numel() < T + 1:
            flags = sim._live_host = torch.zeros(max(T + 1, 64), dtype=torch.int32, pin_memory=True)
            sim._live_events = [torch.cuda.Event() for _ in range(flags.numel())]
            p = ctypes.c_void_p()
            ok = N.lib().craft_host_flag_pointer(flags.data_ptr(), ctypes.byref(p)) == 0
            sim._live_dev = p.value if ok and p.value else 0
        flags[:T + 1].zero_()
        self.host, self.dev, self.events = flags, sim._live_dev, sim._live_events
        self.live = None if self.dev else torch.zeros(T + 1, dtype=torch.int32, device=sim.device)

    def ptr(self, t):
        """Where tick t's kernel stores its flag (the tick's any_live argument)."""
        return self.dev + 4 * t if self.dev else self.live[t].data_ptr()

    def record(self, t):
        """After tick t's launch: the flag's copy to the host where it is not mapped, then the
        tick's event."""
        if not self.dev:
            self.host[t:t + 1].copy_(self.live[t:t + 1], non_blocking=True)
        self.events[t].record()

    def wait(self, t):
        """Blocks until tick t's event has completed; True while some env is still running."""
        self.events[t].synchronize()
        return int(self.host[t]) != 0


class _NoEvent:
    """The per-tick event of a simulator whose calls are synchronous (the CPU variant)."""

    def record(self):
        pass

    def synchronize(self):
        pass


def _distances(sim, task, success, seqs, flags_out):
    """craft_rollout_distances over the rollout's final states: every env's distance, is_get
    (bool) and action count, device tensors [n]; flags_out (two int32 on the device) receives
    the None-success and unreachable-target flags."""
    n, dev = sim.n_envs, sim.device
    task = task.contiguous()
    distances = torch.empty(n, dtype=torch.int32, device=dev)
    is_get = torch.empty(n, dtype=torch.uint8, device=dev)
    n_actions = torch.empty(n, dtype=torch.int32, device=dev)
    sim._check(sim._L.craft_rollout_distances(
        sim._h, task.data_ptr(), success.data_ptr(), seqs.data_ptr(), seqs.shape[0],
        distances.data_ptr(), is_get.data_ptr(), n_actions.data_ptr(), flags_out.data_ptr(),
        sim._stream()), "craft_rollout_distances")
    return distances, is_get.view(torch.bool), n_actions


def _finish(sim, task, success, seqs, t, is_eval, keep_obs, obs_hist, timing, t_start, t_loop,
            t_end_loop, dev):
    """The rollout's summary (imitation.py:79-99) with one read-back: one launch computes every
    env's distance (failed get tasks: find_closest_resources' length on the initial grid at the
    final pose), is_get and action count (craft_rollout_distances); then the episode counters,
    the None-success and unreachable-target flags and the latched-error word come back in one
    transfer."""
    buf = getattr(sim, "_summary_buf", None)
    if buf is None:   # int64 [0:3] stats, [3] the two flags (int32), [4:6] the error word (int32[4])
        buf = sim._summary_buf = torch.zeros(6, dtype=torch.int64, device=dev)
    distances, is_get, n_actions = _distances(sim, task, success, seqs, buf[3:4])
    sim.stats(out=buf[0:3])
    sim.error_word(out=buf[4:6].view(torch.int32))
    summary = buf.cpu()
    flags = summary[3:4].view(torch.int32).tolist()
    _, ended, env_steps = summary[:3].tolist()
    bad_success, unreachable = flags
    err = int(summary[4:6].view(torch.int32)[0])
    if err:
        sim.check()                              # raises: an error latched in the loop or the probe
    if bad_success:
        raise RolloutError("satisfies() returned None for a finished episode (imitation.py:68)")
    if unreachable:
        raise RolloutError("find_closest_resources found no target: len(None) (imitation.py:88-89)")
    num_interactions = 0 if is_eval else env_steps
    num_steps = 0 if is_eval else env_steps - ended
    if timing is not None:
        t_done = time.perf_counter()
        for k, v in (("setup", t_loop - t_start), ("loop", t_end_loop - t_loop),
                     ("summary", t_done - t_end_loop), ("ticks", t)):
            timing[k] = timing.get(k, 0) + v
    return RolloutInfo(action_seqs=seqs[:t], n_actions=n_actions, success=success,
                       distances=distances, is_get=is_get, num_interactions=num_interactions,
                       num_steps=num_steps, ticks=t,
                       obs=obs_hist[:t + 1] if keep_obs else None)


class EvalContext:
    """What evaluate() hands the student beside the observations, int32 device tensors [n]:
    episode (the queue index, i.e. the row of `specs`, each slot runs; -1 when the slot is
    idle), tick (ticks into the slot's current episode) and restarted (1 for a slot that began
    an episode since the last call: a recurrent student clears its state there)."""

    def __init__(self, episode, tick, restarted):
        self.episode, self.tick, self.restarted = episode, tick, restarted


class EvalInfo(_Info):
    """ImitationTrainer.evaluate's results (trainers/imitation.py:183-226): eval_info, the
    reference's dict id -> {'actions', 'success'}; success_rate (per cent) and avg_distance
    (get tasks only) as it logs them; and per instance, in the order of `specs`, host arrays:
    success int8, n_actions int32, action_seqs int32 [count, max_timesteps] (-1 padded),
    distances int32 (-1 where the task is not a get task), end_pose int32 [count, 3] (x, y,
    dir of the final state); ticks = step launches of the pass."""


def _specs_array(specs):
    """A pass's `specs`, the (scenario, x, y, dir, task) arrays or [count, 5] rows, as a
    contiguous int32 host array [count >= 1, 5]."""
    specs = np.ascontiguousarray(np.asarray(torch.as_tensor(_stack_specs(specs)).cpu()),
                                 dtype=np.int32)
    if specs.ndim != 2 or specs.shape[1] != 5 or len(specs) == 0:
        raise ValueError("specs must be [count >= 1, 5]")
    return specs


def _begin_pass(sim, specs, obs=None, wrap=False):
    """Starts one pass over `specs` (a _specs_array): installs them as the episode queue and
    puts slot i on row i, to take rows i + n, i + 2n, ... after it.  Every slot needs a first
    entry, so a split shorter than n_envs is padded with copies of its first row, whose episodes
    the results drop.  Returns the padded queue, count = len(specs) and Q = len(queue)."""
    n, count = sim.n_envs, len(specs)
    queue = specs if count >= n else np.concatenate([specs, np.repeat(specs[:1], n - count, 0)])
    sim.set_episode_queue(torch.as_tensor(queue))
    sim.begin_episodes(first=0, stride=n, wrap=wrap, obs=obs)
    return queue, count, len(queue)


def _pose_xyd(p):
    """end_pose words (x | y << 8 | dir << 16) as (x, y, dir)."""
    return p & 0xff, (p >> 8) & 0xff, (p >> 16) & 3


def _cut_episodes(ended, pose, succ, count, rec=None, T=None):
    """A pass's per-tick records, host arrays [ticks, n] (the queue index of an episode that
    ended at that tick in that slot or -1, its final pose word, its success; rec: the action
    taken), as per-episode results in the order of the queue: length int32 [count], success int8
    [count] (-2: never finished), end_pose int32 [count, 3] and, with rec, the actions int32
    [count, T] padded with -1 (else None).  Slot i runs episodes i, i + n, ... in order, so an
    episode's ticks are those after the slot's previous end, up to its own.  Rows >= count
    (the padding of a short split) are dropped."""
    length = np.zeros(count, dtype=np.int32)
    success = np.full(count, -2, dtype=np.int8)
    end_pose = np.zeros((count, 3), dtype=np.int32)
    seqs = None if rec is None else np.full((count, T), -1, dtype=np.int32)
    tt, ii = np.nonzero(ended >= 0)
    start = np.zeros(ended.shape[1], dtype=np.int64)
    for t, i in zip(tt, ii):                             # (np.nonzero: tick-major, so in order per slot)
        e = ended[t, i]
        if e < count:
            length[e] = t + 1 - start[i]
            success[e] = succ[t, i]
            end_pose[e] = _pose_xyd(pose[t, i])
            if rec is not None:
                seqs[e, :length[e]] = rec[start[i]:t + 1, i]
        start[i] = t + 1
    return length, success, end_pose, seqs


def evaluate(sim, specs, act, ids=None, max_ticks=None, head=None, head_seed=0):
    """One pass over `specs` (ImitationTrainer.evaluate, trainers/imitation.py:183-226): every
    instance is run once, in eval mode, and a slot that finishes one moves straight on to the
    next (the episode queue, craft_step_stream) instead of idling until its batch is done.

    specs: (scenario, x, y, dir, task) arrays, e.g. Dataset.specs(all instances), or int32
      [count, 5] rows.  ids: the instances' ids (default: their indices).
    act(obs, ctx) -> int device tensor [n]: obs is [n, F] on the device in the simulator's obs
      format, overwritten by the next tick; ctx is an EvalContext.  Slot i's episodes are
      specs rows i, i + n, i + 2n, ...: the assignment is static, so results do not depend on
      timing.  The action of an idle slot is ignored (any value in 0..5).
    max_ticks: a bound on the pass (default: ceil(count / n) * max_timesteps, which it cannot
      exceed); RuntimeError if it ends with slots still running.
    head: None, "argmax" or "sample": as do_rollout's, act returns float32 [n, 6] logits and the
      tick chooses the action (craft_step_policy_stream).
    The failed get episodes' distances (imitation.py:83-91: find_closest_resources on the
    initial grid at the final pose) are computed after the pass from the queue entries and the
    recorded final poses (craft_episode_summary): the simulator's slots are left as the pass
    left them.
    Raises RolloutError where the reference raises (success None; no reachable target)."""
    return _queue_pass(sim, specs, act, ids, max_ticks, lang=False, head=head, head_seed=head_seed)


def _queue_pass(sim, specs, act, ids, max_ticks, lang, head=None, head_seed=0):
    """evaluate()'s pass over the queue under either protocol: craft_step_stream (the imitation
    trainer's), or with `lang` craft_step_lang_stream (the language trainers':
    language_rollout.evaluate).  The two argument structs name their shared fields alike.  With a
    head the tick is craft_step_policy_stream / craft_step_lang_policy_stream."""
    n, dev, T = sim.n_envs, sim.device, sim.config.max_timesteps
    specs = _specs_array(specs)
    ids = list(range(len(specs))) if ids is None else list(ids)
    if len(ids) != len(specs):
        raise ValueError(f"{len(ids)} ids for {len(specs)} specs")
    obs = sim.empty_obs()
    _, _, Q = _begin_pass(sim, specs, obs)
    bound = -(-Q // n) * T                                # no slot's stream of episodes is longer
    max_ticks = bound if max_ticks is None else min(int(max_ticks), bound)
    i32 = dict(dtype=torch.int32, device=dev)
    rec = torch.full((max_ticks, n), -1, **i32)
    ended = torch.full((max_ticks, n), -1, **i32)
    pose = torch.full((max_ticks, n), -1, **i32)
    succ = torch.full((max_ticks, n), -1, dtype=torch.int8, device=dev)
    now = torch.empty(n, **i32)
    ctx = EvalContext(torch.arange(n, **i32), torch.zeros(n, **i32), torch.ones(n, **i32))
    live = _LiveFlags(sim, max_ticks)
    what = "craft_step_lang_stream" if lang else "craft_step_stream"
    hd = None
    if head is not None:
        what = "craft_step_lang_policy_stream" if lang else "craft_step_policy_stream"
        hd = _head_struct(head, head_seed)
    args = N.craft_lang_stream_step_args_t() if lang else N.craft_stream_step_args_t()
    args.step.flags = 0 if lang else N.STEP_AUTORESET
    args.step.obs = obs.data_ptr()
    args.episode_now = now.data_ptr()
    fn, h, pargs = getattr(sim._L, what), sim._h, ctypes.byref(args)
    t = 0
    running = True
    while running and t < max_ticks:
        actions = _policy_output(act(obs, ctx), n, dev, head)
        if hd is None:
            args.step.actions = actions.data_ptr()
        else:
            hd.logits = actions.data_ptr()
        args.step.tick = t
        args.step.success = succ[t].data_ptr()
        args.step.action_record = rec[t].data_ptr()
        args.step.any_live = live.ptr(t)
        args.episode_end = ended[t].data_ptr()
        args.end_pose = pose[t].data_ptr()
        if hd is None:
            st = fn(h, pargs, sim._stream())
        elif lang:                                   # (no alt head: an evaluation has one model)
            st = fn(h, pargs, ctypes.byref(hd), None, sim._stream())
        else:
            st = fn(h, pargs, ctypes.byref(hd), sim._stream())
        if st:
            N.check(st, h, what, L=sim._L)
        # the next call's context, on the device
        began = ended[t] >= 0
        ctx = EvalContext(now.clone(), torch.where(began, 0, ctx.tick + 1).to(torch.int32),
                          (began & (now >= 0)).to(torch.int32))
        live.record(t)
        running = live.wait(t)
        t += 1
    if running:
        raise RuntimeError(f"evaluate: slots still running after {t} ticks")
    sim.check()                                  # an error latched during the pass
    return _eval_summary(sim, specs, ids, rec[:t], ended[:t], pose[:t], succ[:t], t,
                         ("primitive_language.py:124", "primitive_language.py:129-131") if lang
                         else ("imitation.py:68", "imitation.py:88-89"))


def _eval_summary(sim, specs, ids, rec, ended, pose, succ, ticks, lines):
    """evaluate()'s per-instance results from the pass's per-tick records (device tensors
    [ticks, n]: the action taken, the queue index of an episode that ended, its final pose and
    success), in one craft_episode_summary call: the records stay on the device and only the
    per-episode results come back.  The same under both protocols: the ending tick's record is
    the episode's last action, and the pose is the final state's (the language protocol's: after
    the ending step).  The simulator's slots are not touched.  lines: where the reference
    raises, for the two messages."""
    count = len(specs)
    out = sim.episode_summary(ended, pose, succ, action_record=rec, count=count)
    n_actions, success, pose_word, distances, seqs, flags = (
        out[k].cpu().numpy() for k in ("length", "success", "end_pose", "distance", "actions", "flags"))
    sim.check()                                  # an entry or a pose out of range in the records
    if (success == -2).any():
        raise RuntimeError(f"evaluate: instance {int(np.argmax(success == -2))} was never finished")
    if flags[0] or (success < 0).any():
        raise RolloutError(f"satisfies() returned None for a finished episode ({lines[0]})")
    end_pose = np.stack(_pose_xyd(pose_word), 1).astype(np.int32)
    goals = np.asarray([t.goal_name == "get" for t in sim.task_manager.tasks])
    is_get = goals[specs[:, 4]]
    if flags[1]:
        raise RolloutError(f"find_closest_resources found no target: len(None) ({lines[1]})")
    # The reference's dict: python ints in one conversion per array, not one per action, and the
    # collector paused meanwhile: three containers per instance, none of them garbage, and its
    # passes over them cost several times the build itself (65,536 instances: 290 against 40 ms).
    collecting = gc.isenabled()
    gc.disable()
    try:
        eval_info = {i: {"actions": a[:k], "success": s}
                     for i, a, k, s in zip(ids, seqs.tolist(), n_actions.tolist(), success.tolist())}
    finally:
        if collecting:
            gc.enable()
    if len(eval_info) != count:
        raise ValueError("ids are not unique (imitation.py:203)")
    get_d = distances[is_get]
    return EvalInfo(eval_info=eval_info, success_rate=int(success.sum()) / count * 100,
                    avg_distance=(int(get_d.sum()) / len(get_d)) if len(get_d) else float("nan"),
                    success=success, n_actions=n_actions, action_seqs=seqs, distances=distances,
                    is_get=is_get, end_pose=end_pose, ticks=ticks)


def _summary_outs(out):
    """What CraftSim.episode_summary returned, as the outputs of the next call over the same
    queue entries (nothing for the first call, which allocates them)."""
    return {k + "_out": v for k, v in out.items() if v is not None}


class ReplayInfo(_Info):
    """replay()'s results, host arrays in the order of `specs`: success int8 (satisfies() of the
    state the episode ended in), length int32 (ticks the device ran the episode for), end_pose
    int32 [count, 3] (x, y, dir of the final state), distances int32 (EvalInfo's: -1 where the
    task is not a get task, 0 for a get episode that did not fail, else
    find_closest_resources' length on the initial grid at the final pose, -1 where it finds no
    target it can reach and -2 where it raises; None on a world the teachers refuse,
    4 * W * H > 1000); ticks and launches of the pass."""


def replay(sim, specs, action_seqs, ticks_per_launch=32, on_chunk=None, epochs=1):
    """One pass over `specs` driven by recorded actions (a dataset's demonstrations, or the
    `actions` of an EvalInfo), K ticks per launch on the episode queue (craft_rollout_replay):
    the (state, action) pairs behaviour cloning trains on, without a launch per tick.

    specs: as evaluate()'s.  action_seqs[e]: episode e's actions, each 0..5, at most
      max_timesteps of them, ending in its only STOP or max_timesteps long; ValueError names the
      first episode that is neither.  Or all of them as one int array or tensor [count, <=
      max_timesteps], each row padded with -1 (DemonstrationInfo.action_seqs,
      EvalInfo.action_seqs).  Under the imitation protocol such an episode takes exactly
      len(action_seqs[e]) ticks, so slot i's action stream is the sequences of episodes i,
      i + n, i + 2n, ... one after the other.  The sequences are installed once beside the queue
      (craft_episode_actions) and every launch reads its own actions on the device: the host
      lays out no action tensor and copies nothing back until the pass is over.
    on_chunk(obs, episode, step, action): called with [K, n, ...] device tensors, first with
      the K = 1 chunk of begin_episodes' observations, then once per launch (the tensors are
      overwritten by the next launch).  obs[k, i] is slot i's state after that tick, in the
      simulator's obs format; episode (int32) the row of `specs` it belongs to, -1 for an idle
      slot; step (int32) how many of that episode's actions were already taken; action (int32)
      the recorded action taken next from that state, action_seqs[episode][step], or -1 for an
      idle slot.  Over the pass the rows with action >= 0 are the (state, action) pairs of
      every sequence, each exactly once per epoch.
    epochs: with epochs > 1 the pass runs that many times over under CRAFT_QUEUE_WRAP, in one
      stream of launches; len(specs) must then be a multiple of n_envs (ValueError), so that a
      slot's stream of episodes repeats as it is.
    Returns a ReplayInfo (of the last end of every episode).  RolloutError if the device ran an
    episode for another number of ticks than its sequence has, or latched an error."""
    n, dev, T = sim.n_envs, sim.device, sim.config.max_timesteps
    K, epochs = int(ticks_per_launch), int(epochs)
    if K < 1:
        raise ValueError("ticks_per_launch must be >= 1")
    if epochs < 1:
        raise ValueError("epochs must be >= 1")
    specs = _specs_array(specs)
    if len(action_seqs) != len(specs):
        raise ValueError(f"{len(action_seqs)} action sequences for {len(specs)} specs")
    if epochs > 1 and len(specs) % n:
        raise ValueError(f"epochs > 1 needs len(specs) to be a multiple of n_envs ({len(specs)} % {n})")
    count = len(action_seqs)
    # every sequence checked in one pass over their concatenation (the first bad episode is named)
    if isinstance(action_seqs, (np.ndarray, torch.Tensor)) and action_seqs.ndim == 2:
        rows = np.asarray(torch.as_tensor(action_seqs).cpu())
        some = rows != -1                                 # a row runs up to its last value that is no padding
        lens = np.where(some.any(1), rows.shape[1] - np.argmax(some[:, ::-1], 1), 0).astype(np.int64)
        flat = rows[np.arange(rows.shape[1])[None] < lens[:, None]].astype(np.int64)
    else:
        try:                                              # (lists or 1-d arrays: no pass of our own over them)
            lens = np.fromiter(map(len, action_seqs), dtype=np.int64, count=count)
            flat = np.concatenate(action_seqs) if lens.sum() else np.zeros(0)
        except (TypeError, ValueError):                   # a 0-d or 2-d entry: flattened, as ever
            lens = np.fromiter((np.size(s) for s in action_seqs), dtype=np.int64, count=count)
            flat = np.concatenate([np.reshape(s, -1) for s in action_seqs]) if lens.sum() else np.zeros(0)
        flat = flat.astype(np.int64)
    ends = np.cumsum(lens)

    def owners(at):                                       # the episodes of positions `at` of flat
        return np.searchsorted(ends, at, side="right")
    outside = np.zeros(count, dtype=bool)
    outside[owners(np.nonzero((flat < 0) | (flat >= N.N_ACTIONS))[0])] = True
    first_stop = np.full(count, T + 1, dtype=np.int64)
    stops = np.nonzero(flat == N.STOP)[0]                 # (in episode order: the first of each is its first)
    who, at = np.unique(owners(stops), return_index=True)
    first_stop[who] = stops[at] - (ends - lens)[who]
    stopped = first_stop <= T
    early = stopped & (first_stop != lens - 1)
    bad = (lens > T) | outside | early | (~stopped & (lens != T))
    if bad.any():
        e = int(np.argmax(bad))
        if lens[e] > T:
            raise ValueError(f"episode {e}: {int(lens[e])} actions, max_timesteps is {T}")
        if outside[e]:
            raise ValueError(f"episode {e}: an action outside 0..{N.N_ACTIONS - 1}")
        if early[e]:
            raise ValueError(f"episode {e}: STOP at step {int(first_stop[e])}, before its end")
        raise ValueError(f"episode {e}: {int(lens[e])} actions without a STOP (max_timesteps is {T})")
    wrap = epochs > 1
    obs0 = sim.empty_obs()
    _, count, Q = _begin_pass(sim, specs, obs0, wrap=wrap)
    # the tape: one -1 padded row per queue entry, the padding entries STOP at once
    length = np.ones(Q, dtype=np.int64)
    length[:count] = lens
    tape = np.full((Q, T), -1, dtype=np.int32)
    tape[:, 0] = N.STOP
    tape[:count][np.arange(T)[None] < lens[:, None]] = flat
    sim.set_episode_actions(torch.as_tensor(tape))
    # ticks of the pass: the longest slot stream (every slot's, under wrap, once per epoch)
    per_slot = np.zeros(n, dtype=np.int64)
    np.add.at(per_slot, np.arange(Q) % n, length)
    total = int(per_slot.max()) * epochs
    limit = torch.as_tensor(per_slot * epochs, device=dev)

    i32 = dict(dtype=torch.int32, device=dev)
    ring = torch.empty((K, n, sim.n_features), dtype=sim.obs_dtype, device=dev) if on_chunk is not None else None
    ended = torch.empty((K, n), **i32)
    pose = torch.empty((K, n), **i32)
    now = torch.empty((K, n), **i32)
    step = torch.empty((K, n), **i32) if on_chunk is not None else None
    nxt = torch.empty((K, n), **i32) if on_chunk is not None else None
    succ = torch.empty((K, n), dtype=torch.int8, device=dev)

    def shown(episode, action):                          # a padding episode's rows are nobody's pairs
        pad = episode >= count
        return (torch.where(pad, -1, episode).to(torch.int32),
                torch.where(pad, -1, action).to(torch.int32))

    if on_chunk is not None:
        first = torch.arange(n, **i32)
        ep0, ac0 = shown(first, torch.as_tensor(tape[:n, 0].copy(), **i32))
        on_chunk(obs0[None], ep0[None], torch.zeros((1, n), **i32), ac0[None])
    # length, success, end_pose and the failed get episodes' distances: one
    # craft_episode_summary call per launch over its records, the episodes that straddle
    # launches carried by `run`; everything stays on the device until the pass is over
    with_dist = 4 * sim.width * sim.height <= 1000       # (the teachers' BFS-queue limit)
    run, summ = torch.zeros(n, **i32), {}
    t0 = launches = 0
    while t0 < total:
        k = min(K, total - t0)
        # tick0 is a multiple of K, so tick t0 + j writes ring slot j
        sim.rollout_replay(k, tick0=t0, obs=ring, success=succ, episode_end=ended, end_pose=pose,
                           episode_now=now, step_now=step, action_next=nxt)
        launches += 1
        summ = sim.episode_summary(ended[:k], pose[:k], succ[:k], count=count, run=run,
                                   episode_now=now[k - 1], distances=with_dist, **_summary_outs(summ))
        if on_chunk is not None:
            episode, action = shown(now[:k], nxt[:k])
            if wrap:                                     # a slot through its epochs early shows as idle
                over = torch.arange(t0 + 1, t0 + k + 1, device=dev)[:, None] >= limit[None]
                episode, action = torch.where(over, -1, episode), torch.where(over, -1, action)
            # an idle slot: episode -1, step 0, action -1, as a padding episode's rows
            on_chunk(ring[:k], episode, torch.where(episode < 0, 0, step[:k]).to(torch.int32), action)
        t0 += k
        last = now[k - 1]
    # the pass's one read-back
    ran, success, pose_word, running = (x.cpu().numpy() for x in
                                        (summ["length"], summ["success"], summ["end_pose"], last >= 0))
    try:
        sim.check()                                      # an error latched during the pass
    except N.CraftError as e:
        raise RolloutError(f"replay: {e}") from e
    if not wrap and running.any():
        raise RolloutError(f"replay: slots still running after {t0} ticks")
    bad = np.nonzero(ran != length[:count])[0]
    if len(bad):
        e = int(bad[0])
        raise RolloutError(f"replay: the device ran episode {e} for {int(ran[e])} ticks, "
                           f"its sequence has {int(length[e])} actions")
    end_pose = np.stack(_pose_xyd(pose_word), 1).astype(np.int32)
    return ReplayInfo(success=success, length=ran, end_pose=end_pose, ticks=t0, launches=launches,
                      distances=summ["distance"].cpu().numpy() if with_dist else None)


class DemonstrationInfo(_Info):
    """demonstrations()'s results, host arrays in the order of `specs`: action_seqs int32
    [count, max_timesteps] (each episode's actions, its STOP included, padded with -1), length
    int32, success int8 (satisfies() of the state the episode ended in), end_pose int32
    [count, 3] (x, y, dir of the final state); ticks and launches of the pass."""

    def actions(self, e):
        """Episode e's action sequence as a list of ints."""
        return [int(a) for a in self.action_seqs[e, :self.length[e]]]


def demonstrations(sim, specs, ticks_per_launch=32):
    """make_data.get_reference_actions (make_data.py:146-152) for a whole list of (scenario,
    start, task) instances in one pass over the episode queue: every slot acts on the teacher's
    label of its current state until the label is STOP, then takes its next instance, K ticks
    per launch (craft_rollout_teach_stream with label_actions).

    specs: as evaluate()'s.  Returns a DemonstrationInfo.  RolloutError names the first instance
    for which the teacher raised, whose episode reached the time limit without a STOP, or whose
    episode ended with its task unsatisfied (the reference's assert state.satisfies(task))."""
    n, dev, T = sim.n_envs, sim.device, sim.config.max_timesteps
    K = int(ticks_per_launch)
    if K < 1:
        raise ValueError("ticks_per_launch must be >= 1")
    _, count, Q = _begin_pass(sim, _specs_array(specs))
    bound = -(-Q // n) * T                                # no slot's stream of episodes is longer
    label_in, _ = sim.teacher()
    i32 = dict(dtype=torch.int32, device=dev)
    labels = torch.empty((K, n), **i32)
    rec = torch.empty((K, n), **i32)
    ended = torch.empty((K, n), **i32)
    pose = torch.empty((K, n), **i32)
    now = torch.empty((K, n), **i32)
    succ = torch.empty((K, n), dtype=torch.int8, device=dev)
    rows = {k: [] for k in ("rec", "ended", "pose", "succ", "now", "labels")}
    raised = np.nonzero(label_in.cpu().numpy() == -2)[0]  # (slot i starts on instance i)
    raised = raised[raised < count]
    first_raise = int(raised[0]) if len(raised) else None
    t0 = launches = 0
    while True:
        if t0 >= bound:
            raise RolloutError(f"demonstrations: slots still running after {t0} ticks")
        # tick0 is a multiple of K, so tick t0 + j writes ring slot j
        sim.rollout_teach_stream(K, tick0=t0, label_actions=True, label_in=label_in, labels=labels,
                                 action_record=rec, success=succ, episode_end=ended, end_pose=pose,
                                 episode_now=now)
        launches += 1
        label_in = labels[K - 1].clone()
        for k, x in (("rec", rec), ("ended", ended), ("pose", pose), ("succ", succ), ("now", now),
                     ("labels", labels)):
            rows[k].append(x.cpu().numpy().copy())
        t0 += K
        if (rows["now"][-1][K - 1] < 0).all():
            break
    rec, ended, pose, succ, now, labels = (np.concatenate(rows[k]) for k in
                                           ("rec", "ended", "pose", "succ", "now", "labels"))
    bad = (labels == -2) & (now >= 0) & (now < count)
    if bad.any():
        e = int(now[bad].min())
        first_raise = e if first_raise is None else min(e, first_raise)
    try:
        sim.check()                                      # an error latched during the pass
    except N.CraftError as e:
        if first_raise is None:
            raise RolloutError(f"demonstrations: {e}") from e
    if first_raise is not None:
        raise RolloutError(f"demonstrations: the teacher raised on instance {first_raise}")

    length, success, end_pose, seqs = _cut_episodes(ended, pose, succ, count, rec, T)
    if (success == -2).any():
        raise RolloutError(f"demonstrations: instance {int(np.argmax(success == -2))} was never finished")
    stopped = seqs[np.arange(count), length - 1] == N.STOP
    wrong = ~stopped | (success != 1)
    if wrong.any():
        e = int(np.argmax(wrong))
        if not stopped[e]:
            raise RolloutError(f"demonstrations: instance {e} reached the time limit "
                               f"({T} steps) without a STOP")
        raise RolloutError(f"demonstrations: instance {e} ended with its task unsatisfied "
                           f"(satisfies() = {int(success[e])})")
    return DemonstrationInfo(action_seqs=seqs, length=length, success=success, end_pose=end_pose,
                             ticks=t0, launches=launches)


class ImitationRollout:
    """ImitationTrainer.do_rollout(batch, world, student, teacher, is_eval) over
    dataset batches (psketch_amd.dataset.Dataset items): one CraftSim per batch
    size, sharing the dataset's scenario pool.

    policy_mix_rate / random: the behaviour-cloning draw of imitation.py:39-41
    (config.trainer.policy_mix, config.random)."""

    def __init__(self, world, pool, device=None, recipes=None, hints=None,
                 max_timesteps=40, policy_mix_rate=1.0, random=None, obs_format="f32"):
        self.obs_format = obs_format
        self.world, self.device = world, device
        self.recipes, self.hints, self.max_timesteps = recipes, hints, max_timesteps
        self.pool = np.asarray(pool, dtype=np.uint8)
        self.policy_mix_rate = policy_mix_rate
        self.random = random
        self._sims = {}

    def sim(self, n):
        s = self._sims.get(n)
        if s is None:
            s = CraftSim(self.world, n_envs=n, device=self.device,
                         pool_capacity=max(1, len(self.pool)), recipes=self.recipes,
                         hints=self.hints, max_timesteps=self.max_timesteps)
            s.load_pool(self.pool)
            s.set_obs_format(self.obs_format)
            self._sims[n] = s
        return s

    def do_rollout(self, batch, act, is_eval, receive=None, keep_obs=False, head=None, head_seed=0):
        from .dataset import Dataset
        sim = self.sim(len(batch))
        spec = Dataset.specs(batch)
        bc = None
        if not is_eval:
            bc = self.random.binomial(1, self.policy_mix_rate, size=len(batch))
        return do_rollout(sim, spec, act, is_eval, behavior_clone=bc, receive=receive,
                          keep_obs=keep_obs, head=head, head_seed=head_seed)

    def evaluate(self, dataset, act, n_envs=32, head=None, head_seed=0):
        """ImitationTrainer.evaluate(dataset, ...) (trainers/imitation.py:183-226): one pass
        over every instance of `dataset` (a Dataset, or any sequence of its items) on a
        simulator of n_envs slots; see evaluate().  Returns an EvalInfo."""
        from .dataset import Dataset
        items = list(dataset)
        return evaluate(self.sim(n_envs), Dataset.specs(items), act, ids=[it["id"] for it in items],
                        head=head, head_seed=head_seed)
