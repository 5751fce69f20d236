"""Batched do_rollout of the reference's three language trainers
(trainers/primitive_language.py:16-143, interactive_primitive_language.py:16-106,
active_primitive_language.py:16-119) on CraftSim slots.

Their shared loop differs from ImitationTrainer.do_rollout in the tick itself: every running
env steps first (STOP too), only then its timer drops and done latches, and success is
satisfies() of the final state.  One craft_step_lang launch (include/craft.h) is that tick for
the whole batch: the step, the protocol bookkeeping, the action / ASK records, the transition
codes PrimitiveLanguageTeacher.describe reads, features() of the new states, the any-live flag
and, when training, the DemonstrationTeacher's label of every new state (the next tick's
instruction).  Per tick the host runs the student's calls, that launch and one read of the
any-live flag (rollout.py's mapped flags); describe() learns the student's action -> word map
sequentially on the host from one action and one code per env.  The summary is
craft_rollout_distances, as for do_rollout.

The student is duck-typed after the reference's students, batched (INTEGRATION.md has the
signatures); `teacher` is a language.PrimitiveLanguageTeacher, whose student_action_map and
draws from the shared RandomState come out as the reference's.
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from .language import WORDS
from .rollout import (EvalContext, EvalInfo, RolloutError, _Info, _LiveFlags,  # noqa: F401
                      _actions, _distances, _head_struct, _policy_output, _queue_pass)

MODES = ("primitive", "interactive", "active")
PAD = "<PAD>"
ASK = 1            # students/active_primitive_language.py:17


class LanguageRolloutInfo(_Info):
    """The rollout's `info` as tensors: action_seqs int32 [T, n] (-1 where the env did not
    act), n_actions int32 [n], success int8 [n] (1 / 0 / -1 for None), distances int32 [n]
    (-1 where the task is not a get task), is_get bool [n], num_interactions, num_steps,
    ticks (of the last pass)."""

    def as_info(self):
        """The reference's info dict (python lists; success keeps None)."""
        A = self.action_seqs.t().cpu().numpy()
        L = self.n_actions.cpu().numpy()
        succ = self.success.cpu().numpy()
        dist = self.distances.cpu().numpy()
        is_get = self.is_get.cpu().numpy()
        return {
            "action_seqs": [[int(a) for a in A[i, :L[i]]] for i in range(len(L))],
            "success": [None if s < 0 else bool(s) for s in succ],
            "distances": [int(d) for d, g in zip(dist, is_get) if g],
            "num_interactions": int(self.num_interactions),
            "num_steps": int(self.num_steps),
        }


class _Pass:
    """One pass of the loop `while not all(done)` from the episodes' initial states: the
    buffers of its ticks and the tick itself."""

    def __init__(self, sim, spec, teach, head=None, head_seed=0):
        n, dev, T = sim.n_envs, sim.device, sim.config.max_timesteps
        self.sim, self.n, self.T = sim, n, T
        self.obs = sim.empty_obs()
        sim.reset(*spec, obs=self.obs)
        self.seqs = torch.full((T, n), -1, dtype=torch.int32, device=dev)
        self.asks = torch.full((T, n), -1, dtype=torch.int8, device=dev)
        self.codes = torch.full((T, n), -1, dtype=torch.int8, device=dev)
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.success = torch.full((n,), -1, dtype=torch.int8, device=dev)
        self.new_labels = torch.empty(n, dtype=torch.int32, device=dev) if teach else None
        self.ticks = 0
        self.live = _LiveFlags(sim, T)
        self.args = N.craft_lang_step_args_t()
        self.args.done = self.done.data_ptr()
        self.args.success = self.success.data_ptr()
        self.args.obs = self.obs.data_ptr()
        if teach:
            self.args.label_out = self.new_labels.data_ptr()
        # with a head: `actions` and `alt` are float32 [n, 6] logits, the call craft_step_lang_policy
        self.head = self.alt_head = None
        if head is not None:
            self.head = _head_struct(head, head_seed)
            self.alt_head = _head_struct(head, alt_seed(head_seed))

    def tick(self, actions, alt=None, use_alt=None):
        """One craft_step_lang launch, then the read of its any-live flag: True while some env
        is still running."""
        t, a, sim = self.ticks, self.args, self.sim
        a.use_alt = None if use_alt is None else use_alt.data_ptr()
        if self.head is not None:
            return self._head_tick(actions, alt)
        a.actions = actions.data_ptr()
        a.alt_actions = None if alt is None else alt.data_ptr()
        a.tick = t
        a.action_record = self.seqs[t].data_ptr()
        a.ask_record = self.asks[t].data_ptr()
        a.transition_code = self.codes[t].data_ptr()
        a.any_live = self.live.ptr(t)
        sim._check(sim._L.craft_step_lang(sim._h, a, sim._stream()), "craft_step_lang")
        self.ticks = t + 1
        self.live.record(t)
        return self.live.wait(t)

    def _head_tick(self, logits, alt_logits):
        t, a, sim = self.ticks, self.args, self.sim
        self.head.logits = logits.data_ptr()
        alt = None
        if alt_logits is not None:
            self.alt_head.logits = alt_logits.data_ptr()
            alt = ctypes.byref(self.alt_head)
        a.tick = t
        a.action_record = self.seqs[t].data_ptr()
        a.ask_record = self.asks[t].data_ptr()
        a.transition_code = self.codes[t].data_ptr()
        a.any_live = self.live.ptr(t)
        sim._check(sim._L.craft_step_lang_policy(sim._h, a, ctypes.byref(self.head), alt, sim._stream()),
                   "craft_step_lang_policy")
        self.ticks = t + 1
        self.live.record(t)
        return self.live.wait(t)


def alt_seed(head_seed):
    """The seed of the instructed model's head in active training: head_seed ^ 1.  The SAMPLE
    draw hashes seed ^ (global env id << 20) ^ tick with tick < 2^20, so flipping bit 0 of the seed
    gives the instructed head the uniform number the main head has at tick ^ 1, never the one it has at this tick:
    the two heads' draws of a tick are distinct hashes."""
    return (int(head_seed) ^ 1) & (2**64 - 1)


def do_language_rollout(sim, spec, student, teacher, is_eval, mode, ref_actions=None, head=None, head_seed=0,
                        ask_threshold=None):
    """One rollout of sim.n_envs episodes under the protocol of the reference's language
    trainer `mode` ("primitive", "interactive" or "active"); returns a LanguageRolloutInfo.

    spec: (scenario, x, y, dir, task), each n_envs ints.  ref_actions (primitive only): each
    env's demonstration, which teacher.instruct turns into its instruction
    (primitive_language.py:26).  Eager loop: no graph capture, no lookahead.
    head: None, "argmax" or "sample".  With a head the student's act / instructed_act return
      float32 [n, 6] logits instead of actions and the tick chooses each env's action itself
      (craft_step_lang_policy), as rollout.do_rollout(head=) does.  In active training the main
      logits go to the head seeded head_seed and the instructed logits to the alt head seeded
      alt_seed(head_seed) = head_seed ^ 1, both under mode `head`; an env acts on the instructed
      head where it asked.
    ask_threshold (active training with a head): the driver computes the ask bits itself,
      sim.policy_ask(main logits, ask_threshold) (the reference student's entropy / log(6) >
      threshold), between the two decodes, and student.act returns the logits alone."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {MODES}")
    if ask_threshold is not None and head is None:
        raise ValueError("ask_threshold needs a head (the ask rule reads the student's logits)")
    if sim.config.max_timesteps <= 0:
        raise ValueError("max_timesteps must be positive")
    n, dev = sim.n_envs, sim.device
    spec = [sim._i32(a, n) for a in spec]
    task = spec[4].contiguous()
    is_eval = bool(is_eval)
    if mode == "primitive":
        return _primitive(sim, spec, task, student, teacher, is_eval, ref_actions, head, head_seed)
    train = not is_eval
    active = mode == "active"
    student.init(n)
    student.set_tasks(task, is_eval)
    p = _Pass(sim, spec, teach=train, head=head, head_seed=head_seed)
    # the teacher's label of every env's current state; a done env keeps its last one
    labels = None
    raised = torch.zeros((), dtype=torch.bool, device=dev)   # the reference's teacher raised
    if train:
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        sim.teacher(action_out=labels)
    instr = torch.full((n,), -1, dtype=torch.int32, device=dev)            # '<PAD>'
    descriptions = [[PAD] for _ in range(n)] if active else [None] * n
    num_interactions = 0
    t = 0
    while True:
        obs = p.obs
        alt = ask = None
        if is_eval:
            actions = _policy_output(student.act(obs, t), n, dev, head)
        elif active:
            if ask_threshold is not None:
                # the main model decodes; the ask bits; the instructions; the instructed model
                actions = _policy_output(student.act(obs, t), n, dev, head)
                ask = sim.policy_ask(actions, ask_threshold) * ASK
            else:
                actions, ask = student.act(obs, t)
                actions = _policy_output(actions, n, dev, head)
            ask = (torch.as_tensor(ask, device=dev).reshape(n) == ASK).to(torch.uint8).contiguous()
            asked = ask != 0
            # the teacher is asked about ASK envs only, done ones included (:51-54)
            raised |= ((labels == -2) & asked).any()
            instr = torch.where(asked, labels, instr)
            student.set_instructions(instr)
            alt = _policy_output(student.instructed_act(obs, t, ask), n, dev, head)
        else:
            raised |= (labels == -2).any()           # asked about every env, done or not (:49-51)
            instr = labels
            student.set_instructions(instr)
            actions = _policy_output(student.instructed_act(obs, t), n, dev, head)
        more = p.tick(actions, alt, ask)
        if train:
            # a slot done before the tick was not labelled (-1): it keeps its last label
            labels = torch.where(p.new_labels == -1, labels, p.new_labels)
        if train or not active:
            # describe every env that stepped (active: that stepped on an instruction), in env
            # order; the others keep their last description (:66-69, active :73-80)
            rec = p.seqs[t].cpu().numpy()
            codes = p.codes[t].cpu().numpy()
            if active:
                arec = p.asks[t].cpu().numpy()
                codes = np.where(arec == 1, codes, -1)
                num_interactions += int((arec == 1).sum())
            else:
                num_interactions += int((codes >= 0).sum()) if train else 0
            for i, w in enumerate(teacher.describe_batch(rec, codes)):
                if w is not None:
                    descriptions[i] = [w]
            if active:
                student.receive(descriptions, ask)
            else:
                student.receive(descriptions)
        student.terminate(p.done)
        t += 1
        if not more:
            break
    if train:
        if active:
            student.set_tasks(task, is_eval)
        student.imitate_instructed()
    num_steps = int((p.seqs[:t] >= 0).sum()) if train else 0
    return _summary(sim, task, p, num_interactions, num_steps, raised)


def evaluate(sim, specs, act, ids=None, max_ticks=None, head=None, head_seed=0):
    """The reference's evaluate of its three language trainers, one pass over `specs`.  They
    inherit ImitationTrainer.evaluate (trainers/primitive_language.py:14, imitation.py:183-226),
    which loops over THEIR do_rollout(..., is_eval=True); in eval mode the three run the same env
    loop (student.act, step, then the timer), so this one function serves them.  It is
    rollout.evaluate on craft_step_lang_stream: the same arguments, the same EvalContext for
    `act` (episode, tick, restarted), the same static slot assignment (slot i runs rows i,
    i + n, ...), the same padding of a split shorter than n_envs, and it returns an EvalInfo.
    What differs is the protocol: an episode that times out takes max_timesteps steps, the
    ending tick steps like any other, success is satisfies() of the state that step left, and a
    failed get episode's distance is measured from the pose after it (end_pose), on the
    initial grid (primitive_language.py:121-133).  Per instance the results equal
    do_language_rollout(is_eval=True) on any batching; no slot idles until the slowest env of
    its batch is done.

    A training loop that feeds a student an endless stream of fresh episodes drives the same
    tick itself, with wrap=True, and reads what do_language_rollout reads per tick:

        sim.set_episode_queue(specs)
        obs = sim.empty_obs()
        sim.begin_episodes(wrap=True, obs=obs)
        labels, _ = sim.teacher()                      # the instruction for every initial state
        new = torch.empty_like(labels)
        rec = torch.empty(n, dtype=torch.int32, device=dev)
        codes = torch.empty(n, dtype=torch.int8, device=dev)
        ended = torch.empty(n, dtype=torch.int32, device=dev)
        for t in range(steps):
            actions, ask = student.act(obs, t)         # the active student's own action and ASK bit
            student.set_instructions(labels)           # (a -2 label: the reference's teacher raised)
            follow = student.instructed_act(obs, t, ask)
            sim.step_lang_stream(actions, tick=t, alt_actions=follow, use_alt=ask, obs=obs,
                                 labels=new, action_record=rec, transition_code=codes,
                                 episode_end=ended)
            # rec / codes -> PrimitiveLanguageTeacher.describe_batch, as in do_language_rollout;
            # ended >= 0: the slot began a new episode, `obs` and `new` are its initial state's
            labels = new.clone()                       # every slot runs on: no -1 under wrap

    Under wrap no slot freezes, so every label is the teacher's answer for the state the student
    sees next, a restarted slot's for its new task.

    head: None, "argmax" or "sample": act returns float32 [n, 6] logits and the tick chooses the
    action (craft_step_lang_policy_stream), as rollout.evaluate(head=) does; with logits the loop
    above calls sim.step_lang_stream(logits=..., alt_logits=..., use_alt=ask, ...)."""
    return _queue_pass(sim, specs, act, ids, max_ticks, lang=True, head=head, head_seed=head_seed)


def _primitive(sim, spec, task, student, teacher, is_eval, ref_actions, head=None, head_seed=0):
    n, dev = sim.n_envs, sim.device
    if ref_actions is None or len(ref_actions) != n:
        raise ValueError("primitive mode needs ref_actions, one action sequence per env")
    instructions = [teacher.instruct(None, ra) for ra in ref_actions]
    L = max(1, max(len(w) for w in instructions))
    instr = np.full((n, L), -1, dtype=np.int32)
    for i, ws in enumerate(instructions):
        instr[i, :len(ws)] = [WORDS.index(w) for w in ws]
    instr = torch.as_tensor(instr, device=dev)
    student.init(n)
    student.set_tasks(task, is_eval)
    student.set_instructions(instr)
    num_interactions = 0 if is_eval else sum(len(w) for w in instructions)
    raised = torch.zeros((), dtype=torch.bool, device=dev)

    def run(instructed):
        p = _Pass(sim, spec, teach=False, head=head, head_seed=head_seed)
        while True:
            t = p.ticks
            act = student.instructed_act if instructed else student.act
            more = p.tick(_policy_output(act(p.obs, t), n, dev, head))
            student.terminate(p.done)
            if not more:
                return p

    p = run(not is_eval)
    num_steps = 0
    if not is_eval:
        num_steps = int((p.seqs[:p.ticks] >= 0).sum())
        # whole-sequence describe per env, in env order (:69-75)
        A = p.seqs[:p.ticks].t().cpu().numpy()
        C = p.codes[:p.ticks].t().cpu().numpy()
        descriptions = []
        for i in range(n):
            k = int((A[i] >= 0).sum())
            descriptions.append(teacher.describe_codes(A[i, :k], C[i, :k]))
        student.receive(descriptions)
        # the second decoding, without exploration, from the same initial states (:77-119)
        student.set_instructions(instr)
        student.reset_history()
        p = run(True)
        student.imitate_instructed()
    return _summary(sim, task, p, num_interactions, num_steps, raised)


def _summary(sim, task, p, num_interactions, num_steps, raised):
    """success / distances of the final states (primitive_language.py:121-133) with one
    read-back: craft_rollout_distances, the flags and the latched-error word."""
    dev, t = sim.device, p.ticks
    buf = torch.zeros(4, dtype=torch.int32, device=dev)   # [0:2] the two flags, [2] raised
    err = torch.zeros(4, dtype=torch.int32, device=dev)
    distances, is_get, n_actions = _distances(sim, task, p.success, p.seqs, buf[0:2])
    buf[2] = raised.to(torch.int32)
    sim.error_word(out=err)
    host = torch.cat([buf, err]).cpu().tolist()
    if host[4]:
        sim.check()                                  # raises: an error latched in the loop
    if host[2]:
        raise RolloutError("the teacher raised on the final state of an env that ended while "
                           "others were still running")
    if host[1]:
        raise RolloutError("find_closest_resources found no target: len(None) "
                           "(primitive_language.py:129-131)")
    return LanguageRolloutInfo(action_seqs=p.seqs[:t], n_actions=n_actions, success=p.success,
                               distances=distances, is_get=is_get,
                               num_interactions=num_interactions, num_steps=num_steps, ticks=t)
