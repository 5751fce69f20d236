"""Generates tests/golden/language_rollout.npz by running the REFERENCE's own do_rollout of its
three language trainers (trainers/primitive_language.py, interactive_primitive_language.py,
active_primitive_language.py) with its own teachers and a table-driven stub student.

Run where the reference is available (see make_golden.py, whose helpers this imports):
    python tests/golden/make_golden_language_rollout.py

Setup: 12x12 worlds, 3x3 windows, 96 envs over the first 16 grids of scenarios_seed123.npz,
get / make tasks, each trainer in train and eval, max_timesteps 40 and 12: 12 cases, each
with a fresh teacher and config.random = RandomState(77).

The stub student is a pure function of three stored tables, [40][96] each:
    policy[t][i]  the action it takes on its own (STOP rare)
    follow[t][i]  instructed_act takes the instruction's action where there is one, else
                  the policy's
    ask[t][i]     the active student's ASK bit
Per case the file keeps action_seqs, success (-1 for None), distances, the two counts, the
instructions and descriptions exactly as the student received them, the teacher's final
student_action_map and config.random's MT19937 state after the rollout.
"""
import contextlib
import io
import os

import numpy as np

import make_golden as G

OUT = G.OUT
WORDS = ["down", "up", "left", "right", "use", "stop"]      # word index = action index
N_ENVS, N_GRIDS, T_MAX = 96, 16, 40
SEED = 77


def widx(w):
    return -1 if w is None or w == "<PAD>" else WORDS.index(str(w))


class _Model:
    def eval(self):
        pass


class Stub:
    """The three reference students' rollout protocol around the tables."""
    ASK = 1

    def __init__(self, mode, policy, follow, ask):
        self.mode, self.policy, self.follow, self.ask = mode, policy, follow, ask
        self.instructed_model = _Model()

    # -- primitive: init(tasks, instructions, states, is_eval); the others: init(states)
    def init(self, *a):
        self.t = 0
        self.instr_log, self.desc_log = [], []
        self.is_eval = None
        if self.mode == "primitive":
            _, instructions, _, self.is_eval = a
            self.instructions = [list(x) for x in instructions]
            self.init_instructions = [list(x) for x in instructions]

    def set_tasks(self, tasks, is_eval):
        self.is_eval = is_eval

    def set_instructions(self, instructions, is_eval=None):
        if self.mode == "primitive":
            assert [list(x) for x in instructions] == self.init_instructions
            return
        self.instructions = [list(x) for x in instructions]
        self.instr_log.append([widx(x[0]) for x in self.instructions])

    def reset_history(self):
        pass

    def terminate(self, i):
        pass

    def imitate_instructed(self):
        pass

    def receive(self, descriptions, ask_actions=None):
        if self.mode == "primitive":
            self.desc_log = [[widx(w) for w in d] for d in descriptions]
        else:
            self.desc_log.append([-1 if d is None else widx(d[0]) for d in descriptions])

    def act(self, states, t=None):
        if self.mode == "primitive":
            return [int(a) for a in self.policy[t]]
        a = [int(x) for x in self.policy[self.t]]
        if self.mode == "active" and not self.is_eval:
            return a, [int(x) for x in self.ask[self.t]]       # t advances in instructed_act
        self.t += 1
        return a

    def instructed_act(self, states, t=None):
        # (active: the second argument is ask_actions, which the stub does not need)
        if self.mode == "primitive":
            out = []
            for i in range(len(states)):
                ins = self.instructions[i]
                out.append(WORDS.index(ins[t]) if self.follow[t][i] and t < len(ins)
                           else int(self.policy[t][i]))
            return out
        t = self.t
        out = []
        for i in range(len(states)):
            w = widx(self.instructions[i][0])
            out.append(w if self.follow[t][i] and w >= 0 else int(self.policy[t][i]))
        self.t += 1
        return out


def make_tables():
    rng = np.random.RandomState(2024)
    policy = rng.randint(0, 5, size=(T_MAX, N_ENVS))
    policy[rng.uniform(size=policy.shape) < 0.02] = 5            # STOP rare
    follow = rng.uniform(size=policy.shape) < 0.7
    follow[:, 5::8] = False                                      # some envs never follow
    follow[:, 6::8] = True                                       # and some always
    ask = rng.uniform(size=policy.shape) < 0.5
    ask[:, 3::11] = False                                        # envs that never ask
    return policy.astype(np.int8), follow.astype(np.uint8), ask.astype(np.uint8)


def load_trainers():
    import trainers
    return {"primitive": trainers.PrimitiveLanguageTrainer,
            "interactive": trainers.InteractivePrimitiveLanguageTrainer,
            "active": trainers.ActivePrimitiveLanguageTrainer}


def main():
    grids = np.load(os.path.join(OUT, "scenarios_seed123.npz"))["w12_grids"][:N_GRIDS]
    policy, follow, ask = make_tables()
    cfg0, world = G.make_world(12, 3)
    tm = G.TaskManager(cfg0)
    K, W = world.cookbook.n_kinds, 12
    task_objs = list(tm.tasks)
    task_ids = [i for i, t in enumerate(task_objs) if t.goal_name in ("get", "make")]
    demo_teacher = G.teachers.load(cfg0)                         # DemonstrationTeacher
    rng = np.random.RandomState(9)
    batch, spec, refs = [], [], []
    for e in range(N_ENVS):
        sc = e % N_GRIDS
        g = grids[sc].reshape(W, W)
        free = [(x, y) for x in range(1, W - 1) for y in range(1, W - 1) if g[x, y] == 0]
        x, y = free[rng.randint(len(free))]
        tk = task_ids[rng.randint(len(task_ids))]
        onehot = G.ids_to_onehot(g, K)
        # the demonstration, as make_data.get_reference_actions builds it
        st = world.init_state(onehot, (x, y))
        ra = [demo_teacher(task_objs[tk], st)]
        while ra[-1] != world.actions.STOP.index:
            _, st = st.step(ra[-1])
            ra.append(demo_teacher(task_objs[tk], st))
        batch.append({"task": task_objs[tk], "grid": onehot, "init_pos": (x, y), "ref_actions": ra})
        spec.append([sc, x, y, 0, tk])
        refs.append(ra)
    L = max(len(r) for r in refs)
    R = np.full((N_ENVS, L), -1, dtype=np.int8)
    for i, r in enumerate(refs):
        R[i, :len(r)] = r
    arrays = {"pool": grids.astype(np.uint8), "spec": np.asarray(spec, dtype=np.int32),
              "policy": policy, "follow": follow, "ask": ask, "ref_actions": R}
    trainers = load_trainers()
    seen = {k: False for k in ("timer_nonidle", "stop", "get_true", "get_false", "rng", "never_asked")}
    for mode in ("primitive", "interactive", "active"):
        for T in (40, 12):
            for is_eval in (False, True):
                cfg = G.make_config()
                cfg.trainer.max_timesteps = T
                cfg.teacher = G.util.Struct(name="PrimitiveLanguageTeacher" if mode == "primitive"
                                            else "InteractivePrimitiveLanguageTeacher")
                cfg.random = np.random.RandomState(SEED)
                key0 = cfg.random.get_state()
                teacher = G.teachers.load(cfg)
                student = Stub(mode, policy, follow, ask)
                trainer = trainers[mode](cfg)
                with contextlib.redirect_stdout(io.StringIO()):
                    info = trainer.do_rollout(batch, world, student, teacher, is_eval)
                key = f"{mode}_{'eval' if is_eval else 'train'}_{T}"
                A = np.full((N_ENVS, T), -1, dtype=np.int8)
                for i, a in enumerate(info["action_seqs"]):
                    A[i, :len(a)] = a
                succ = np.asarray([-1 if s is None else int(bool(s)) for s in info["success"]], dtype=np.int8)
                arrays[key + "_action_seqs"] = A
                arrays[key + "_success"] = succ
                arrays[key + "_distances"] = np.asarray(info["distances"], dtype=np.int16)
                arrays[key + "_counts"] = np.asarray([info["num_interactions"], info["num_steps"]], dtype=np.int64)
                if mode == "primitive":
                    D = np.full((N_ENVS, T), -1, dtype=np.int8)
                    for i, d in enumerate(student.desc_log):
                        D[i, :len(d)] = d
                    arrays[key + "_descriptions"] = D
                else:
                    arrays[key + "_instructions"] = np.asarray(student.instr_log, dtype=np.int8).reshape(-1, N_ENVS)
                    arrays[key + "_descriptions"] = np.asarray(student.desc_log, dtype=np.int8).reshape(-1, N_ENVS)
                m = sorted((int(k), WORDS.index(v)) for k, v in teacher.student_action_map.items())
                arrays[key + "_map"] = np.asarray(m, dtype=np.int8).reshape(-1, 2)
                st = cfg.random.get_state()
                arrays[key + "_mt_key"] = np.asarray(st[1], dtype=np.uint32)
                arrays[key + "_mt_pos"] = np.asarray([st[2]], dtype=np.int32)
                # ---- the cases that tell the protocols apart ----
                if (st[2] != key0[2]) or (st[1] != key0[1]).any():
                    seen["rng"] = True
                gi = 0
                for i in range(N_ENVS):
                    seq = info["action_seqs"][i]
                    state = world.init_state(batch[i]["grid"], batch[i]["init_pos"])
                    prev = state
                    for a in seq:
                        prev = state
                        _, state = state.step(a)
                    if seq[-1] == 5:
                        seen["stop"] = True
                    elif len(seq) == T and (tuple(state.pos) != tuple(prev.pos)
                                            or (state.inventory != prev.inventory).any()):
                        seen["timer_nonidle"] = True
                    if batch[i]["task"].goal_name == "get":
                        d = info["distances"][gi]
                        gi += 1
                        if succ[i] == 1:
                            seen["get_true"] = True
                        elif d > 0:
                            seen["get_false"] = True
                    if mode == "active" and not is_eval and not ask[:len(seq), i].any():
                        seen["never_asked"] = True
                print(key, "ticks", max(len(a) for a in info["action_seqs"]), "success", int((succ == 1).sum()),
                      "counts", arrays[key + "_counts"], "map", m, "mt_pos", st[2])
    missing = [k for k, v in seen.items() if not v]
    assert not missing, f"the fixture lacks the cases {missing}"
    path = os.path.join(OUT, "language_rollout.npz")
    np.savez_compressed(path, **arrays)
    print("language_rollout.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
