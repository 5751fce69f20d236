"""Shared by tests/test_language_rollout_cpu.py and tests/test_gpu_step_lang.py: the cases of
tests/golden/language_rollout.npz (the reference's three language trainers' do_rollout, run by
tests/golden/make_golden_language_rollout.py), the batched table-driven student and the check
of one case against do_language_rollout on any CraftSim."""
import numpy as np
import torch

from psketch_amd import CraftSim, PrimitiveLanguageTeacher, do_language_rollout
from psketch_amd.language import WORDS

WORLD = "craft_medium_12x12"
CASES = [(mode, is_eval, T) for mode in ("primitive", "interactive", "active")
         for T in (40, 12) for is_eval in (False, True)]
CASE_IDS = [f"{m}-{'eval' if e else 'train'}-{T}" for m, e, T in CASES]
SEED = 77            # config.random of every case (make_golden_language_rollout.py)


def _widx(w):
    return -1 if w is None or w == "<PAD>" else WORDS.index(w)


class TableStudent:
    """The batched student protocol as a pure function of the fixture's
    policy / follow / ask tables; logs every instruction and description it is given."""

    def __init__(self, fx, mode, dev):
        self.mode = mode
        self.policy = torch.as_tensor(fx["policy"].astype(np.int32), device=dev)
        self.follow = torch.as_tensor(fx["follow"], device=dev).bool()
        self.ask = torch.as_tensor(fx["ask"], device=dev)
        self.calls = []

    def init(self, n):
        self.n = n
        self.labels = None
        self.instr_log, self.desc_log, self.terminated = [], [], 0
        self.calls.append("init")

    def set_tasks(self, task_ids, is_eval):
        assert task_ids.shape == (self.n,)
        self.is_eval = is_eval
        self.calls.append("set_tasks")

    def set_instructions(self, labels):
        assert labels.dtype == torch.int32
        self.labels = labels
        if self.mode == "primitive":
            self.calls.append("set_instructions")
        else:
            self.instr_log.append(labels.cpu().numpy().copy())

    def act(self, obs, t):
        assert obs.shape[0] == self.n
        if self.mode == "active" and not self.is_eval:
            return self.policy[t], self.ask[t]
        return self.policy[t]

    def instructed_act(self, obs, t, ask=None):
        assert (ask is not None) == (self.mode == "active")
        lab = self.labels
        if lab.dim() == 2:                       # primitive: word t of the env's instruction
            lab = lab[:, t] if t < lab.shape[1] else torch.full_like(lab[:, 0], -1)
        return torch.where(self.follow[t] & (lab >= 0), lab, self.policy[t])

    def receive(self, descriptions, ask=None):
        assert (ask is not None) == (self.mode == "active")
        if self.mode == "primitive":
            self.desc_log = [[_widx(w) for w in d] for d in descriptions]
            self.calls.append("receive")
        else:
            self.desc_log.append([-1 if d is None else _widx(d[0]) for d in descriptions])

    def terminate(self, done):
        assert done.shape == (self.n,)
        self.terminated += 1

    def reset_history(self):
        self.calls.append("reset_history")

    def imitate_instructed(self):
        self.calls.append("imitate_instructed")


def make_sim(fx, T, device):
    sim = CraftSim(WORLD, n_envs=len(fx["spec"]), device=device, pool_capacity=len(fx["pool"]),
                   max_timesteps=T)
    sim.load_pool(fx["pool"])
    return sim


def check_case(fx, sim, mode, is_eval, T):
    """Runs one fixture case through do_language_rollout on `sim` and checks every stored
    array, the teacher's action map and the shared RandomState."""
    key = f"{mode}_{'eval' if is_eval else 'train'}_{T}"
    n = sim.n_envs
    rng = np.random.RandomState(SEED)
    teacher = PrimitiveLanguageTeacher(rng)
    student = TableStudent(fx, mode, sim.device)
    refs = [[int(a) for a in r if a >= 0] for r in fx["ref_actions"]] if mode == "primitive" else None
    info = do_language_rollout(sim, fx["spec"].T.copy(), student, teacher, is_eval, mode,
                               ref_actions=refs)
    sim.check()
    out = info.as_info()
    A = fx[key + "_action_seqs"]
    assert out["action_seqs"] == [[int(a) for a in row if a >= 0] for row in A]
    assert out["success"] == [None if s < 0 else bool(s) for s in fx[key + "_success"]]
    assert out["distances"] == [int(d) for d in fx[key + "_distances"]]
    assert [out["num_interactions"], out["num_steps"]] == [int(c) for c in fx[key + "_counts"]]
    ticks = max(len(a) for a in out["action_seqs"])
    assert info.ticks == ticks and student.terminated == ticks * (1 if is_eval or mode != "primitive" else 2)
    if mode == "primitive":
        if not is_eval:
            D = fx[key + "_descriptions"]
            assert student.desc_log == [[int(w) for w in row if w >= 0] for row in D]
            assert student.calls == ["init", "set_tasks", "set_instructions", "receive",
                                     "set_instructions", "reset_history", "imitate_instructed"]
        else:
            assert student.calls == ["init", "set_tasks", "set_instructions"]
    else:
        I, D = fx[key + "_instructions"], fx[key + "_descriptions"]
        got_i = np.asarray(student.instr_log, dtype=np.int64).reshape(-1, n)
        got_d = np.asarray(student.desc_log, dtype=np.int64).reshape(-1, n)
        np.testing.assert_array_equal(got_i, I)
        np.testing.assert_array_equal(got_d, D)
        assert student.calls[-1] == ("imitate_instructed" if not is_eval else "set_tasks")
    m = sorted((int(k), WORDS.index(v)) for k, v in teacher.student_action_map.items())
    assert m == [tuple(int(x) for x in r) for r in fx[key + "_map"]]
    st = rng.get_state()
    np.testing.assert_array_equal(np.asarray(st[1], dtype=np.uint32), fx[key + "_mt_key"])
    assert st[2] == int(fx[key + "_mt_pos"][0])
    return info


def check_teacher_raise_of_ended_slot(device, n=70, **tune_teach):
    """Where the reference's teacher raises (a reachable target, then an unreachable one:
    len(None), teachers/base.py:31) the label is -2; craft_step_lang latches CRAFT_ETEACHER for
    a slot still running after the tick, not for one whose episode the tick ended."""
    from psketch_amd import _native as N

    def sim_on_raising_state():
        sim = CraftSim(WORLD, n_envs=n, device=device, pool_capacity=1)
        ix = sim.cookbook.index
        g = np.zeros((12, 12), dtype=np.uint8)
        g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = ix["boundary"]
        g[3, 3] = g[7, 7] = ix["wood"]                       # (3, 3) reachable, (7, 7) walled in
        g[6, 7] = g[8, 7] = g[7, 6] = g[7, 8] = ix["stone"]
        sim.load_pool(g[None])
        if tune_teach:
            sim.tune_teach(**tune_teach)
        task = sim.task_manager["get[wood]"].id
        z = np.zeros(n, dtype=np.int32)
        sim.reset(z, z + 9, z + 2, z, z + task)
        return sim

    dev = "cpu" if device == "cpu" else "cuda"
    labels = torch.zeros(n, dtype=torch.int32, device=dev)
    done = torch.zeros(n, dtype=torch.uint8, device=dev)
    sim = sim_on_raising_state()
    sim.step_lang(torch.full((n,), N.STOP, dtype=torch.int32, device=dev), labels=labels, done=done)
    sim.check()                                              # nothing latched
    assert bool((labels == -2).all()) and bool((done == 1).all())
    sim = sim_on_raising_state()
    acts = torch.full((n,), N.STOP, dtype=torch.int32, device=dev)
    acts[n - 3] = N.LEFT
    sim.step_lang(acts, labels=labels, done=done)
    assert bool((labels == -2).all()) and int(done.sum()) == n - 1
    try:
        sim.check()
    except N.CraftError as e:
        assert e.status == N.ETEACHER
    else:
        raise AssertionError("a running slot whose teacher raises must latch CRAFT_ETEACHER")
