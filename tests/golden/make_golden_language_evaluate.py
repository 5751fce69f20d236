"""Generates tests/golden/language_evaluate.npz by running the REFERENCE's own evaluate of its three
language trainers (PrimitiveLanguageTrainer, InteractivePrimitiveLanguageTrainer and
ActivePrimitiveLanguageTrainer inherit ImitationTrainer.evaluate, trainers/imitation.py:183-226,
which loops over THEIR do_rollout(..., is_eval=True)) over the first 150 instances of its dev split
(data/craft_medium_dev.json, in dataset order), batch size 32, max_timesteps 12, with its own
teachers and dataset class and a table-driven stub student in eval mode.

Run where the reference is available (see make_golden.py, whose helpers this imports):
    python tests/golden/make_golden_language_evaluate.py

The table is make_golden_evaluate.py's recipe: table[i][t] is the action instance i takes at tick
t of its episode, its own ref_actions (STOP after their end), except that every fourth instance
takes a seeded draw instead (RandomState(3), STOP at 15 %).  The stub is
make_golden_language_rollout.py's three students' protocol in eval mode around that table.

In eval mode the three trainers run the same env loop, so the generator asserts that they return
the same actions, success and distances, and keeps one copy: the ids, the table, and per instance
the action sequence and success, the success rate evaluate() returned and the mean distance it
logged.  It asserts at least 10 each of: successes, failures, failed get tasks with a distance
> 0, episodes ended by the time limit, episodes ended by STOP, and prints how many instances
differ from imitation_evaluate.npz (the other protocol on the same table).
"""
import contextlib
import io
import os

import numpy as np

import make_golden as G
from make_golden_evaluate import BATCH, N_INSTANCES, SEED, STOP, T_MAX, Batches
from make_golden_language_rollout import _Model, load_trainers

OUT = G.OUT


class Stub:
    """The three reference students' rollout protocol, eval mode only, around the table."""
    ASK = 1

    def __init__(self, mode, table, index_of):
        self.mode, self.table, self.index_of = mode, table, index_of
        self.batch = None                       # set by Batches before each do_rollout
        self.instructed_model = _Model()

    # -- primitive: init(tasks, instructions, states, is_eval); the others: init(states)
    def init(self, *a):
        self.t = 0
        if self.mode == "primitive":
            assert a[3] and len(a[2]) == len(self.batch)
        else:
            assert len(a[0]) == len(self.batch)

    def set_tasks(self, tasks, is_eval):
        assert is_eval

    def receive(self, descriptions, ask_actions=None):
        pass

    def terminate(self, i):
        pass

    def act(self, states, t=None):
        if self.mode == "primitive":
            assert t == self.t
        t = min(self.t, T_MAX - 1)
        self.t += 1
        return [int(self.table[self.index_of[item["id"]], t]) for item in self.batch]


def main():
    from data.dataset import Dataset
    _, world = G.make_world()
    trainers = load_trainers()
    results = {}
    for mode in ("primitive", "interactive", "active"):
        cfg = G.make_config()
        cfg.data_dir = "data"
        cfg.trainer.batch_size = BATCH
        cfg.trainer.max_timesteps = T_MAX
        cfg.teacher = G.util.Struct(name="PrimitiveLanguageTeacher" if mode == "primitive"
                                    else "InteractivePrimitiveLanguageTeacher")
        cfg.random = np.random.RandomState(77)
        tm = G.TaskManager(cfg)
        teacher = G.teachers.load(cfg)
        ds = Dataset(cfg, "dev", tm)
        ds.data = ds.data[:N_INSTANCES]
        ds.instance_by_id = {item["id"]: item for item in ds.data}
        ids = [item["id"] for item in ds.data]
        rng = np.random.RandomState(SEED)
        table = np.full((N_INSTANCES, T_MAX), STOP, dtype=np.int8)
        for i, item in enumerate(ds.data):
            ref = list(item["ref_actions"])[:T_MAX]
            table[i, :len(ref)] = ref
            if i % 4 == 0:
                table[i] = rng.choice(6, size=T_MAX, p=[.17, .17, .17, .17, .17, .15])
        stub = Stub(mode, table, {iid: i for i, iid in enumerate(ids)})
        trainer = trainers[mode](cfg)
        distances = []
        rollout = trainer.do_rollout

        def recording_rollout(*a, **kw):
            info = rollout(*a, **kw)
            distances.extend(info["distances"])
            return info
        trainer.do_rollout = recording_rollout
        with contextlib.redirect_stdout(io.StringIO()):
            success_rate, eval_info = trainer.evaluate(Batches(ds, stub), world, stub, teacher)
        actions = np.full((N_INSTANCES, T_MAX), -1, dtype=np.int8)
        success = np.zeros(N_INSTANCES, dtype=np.int8)
        for i, iid in enumerate(ids):
            a = eval_info[iid]["actions"]
            actions[i, :len(a)] = a
            success[i] = eval_info[iid]["success"]
        is_get = np.asarray([item["task"].goal_name == "get" for item in ds.data])
        assert len(distances) == int(is_get.sum())
        # (evaluate() shuffles the batches through config.random: the distances are compared sorted)
        results[mode] = dict(ids=np.asarray(ids), table=table, actions=actions, success=success,
                             success_rate=float(success_rate), avg_distance=sum(distances) / len(distances),
                             distances=sorted(distances))
    first = results["primitive"]
    for mode, r in results.items():
        for k in first:
            assert np.array_equal(r[k], first[k]), (mode, k)
    actions, success = first["actions"], first["success"]
    n_act = (actions >= 0).sum(1)
    last = actions[np.arange(N_INSTANCES), n_act - 1]
    stops = int((last == STOP).sum())
    timeouts = int(((last != STOP) & (n_act == T_MAX)).sum())
    assert stops + timeouts == N_INSTANCES
    counts = {"successes": int(success.sum()), "failures": int((success == 0).sum()),
              "failed get tasks with distance > 0": int(sum(d > 0 for d in first["distances"])),
              "timeouts": timeouts, "STOP endings": stops}
    print(counts, "success rate", first["success_rate"], "mean distance", first["avg_distance"])
    for k, v in counts.items():
        assert v >= 10, (k, v)
    other = np.load(os.path.join(OUT, "imitation_evaluate.npz"))
    assert np.array_equal(other["table"], first["table"]) and np.array_equal(other["ids"], first["ids"])
    differ = (other["actions"] != actions).any(1) | (other["success"] != success)
    print("instances that differ from imitation_evaluate.npz:", int(differ.sum()), "of", N_INSTANCES,
          "(success:", int((other["success"] != success).sum()), ")")
    path = os.path.join(OUT, "language_evaluate.npz")
    np.savez_compressed(path, ids=first["ids"], table=first["table"], actions=actions, success=success,
                        success_rate=np.float64(first["success_rate"]), avg_distance=np.float64(first["avg_distance"]),
                        max_timesteps=np.int32(T_MAX), batch_size=np.int32(BATCH))
    print("language_evaluate.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
