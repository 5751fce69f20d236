"""Generates tests/golden/imitation_evaluate.npz by running the REFERENCE's own
ImitationTrainer.evaluate (trainers/imitation.py:183-226) over the first 150 instances of its dev
split (data/craft_medium_dev.json, in dataset order), batch size 32, max_timesteps 12, with its own
DemonstrationTeacher and dataset class and a table-driven stub student.

Run where the reference is available (see make_golden.py, whose helpers this imports):
    python tests/golden/make_golden_evaluate.py

The stub student is a pure function of (instance, episode tick): table[i][t] is the action
instance i takes at tick t of its episode, its own ref_actions (STOP after their end), except
that every fourth instance (i % 4 == 0) takes a seeded draw instead (RandomState(SEED), STOP at
15 %).  evaluate() shuffles the instances through config.random; the table does not care.

The file keeps the ids, the table, and per instance the action sequence and success evaluate()
returned, the success rate it returned and the mean distance it logged (recomputed here from the
distances of the do_rollout calls it made).  The generator asserts that the fixture holds at
least 10 each of: successes, failures, failed get tasks with a distance > 0, episodes ended by
the time limit, episodes ended by STOP.
"""
import contextlib
import io
import os

import numpy as np

import make_golden as G

OUT = G.OUT
N_INSTANCES, BATCH, T_MAX = 150, 32, 12
SEED = 3
STOP = 5


class Stub:
    """students/imitation.py's rollout protocol (init / act) around the table."""

    def __init__(self, table, index_of):
        self.table, self.index_of = table, index_of
        self.batch = None                       # set by Batches before each do_rollout

    def init(self, tasks, states, is_eval):
        assert is_eval and len(states) == len(self.batch)
        self.t = 0

    def act(self, states):
        t = min(self.t, T_MAX - 1)
        self.t += 1
        return [int(self.table[self.index_of[item["id"]], t]) for item in self.batch]


class Batches:
    """The reference's dataset, telling the stub which instances the next do_rollout holds."""

    def __init__(self, dataset, stub):
        self.dataset, self.stub, self.split = dataset, stub, dataset.split

    def iterate_batches(self):
        for batch in self.dataset.iterate_batches():
            self.stub.batch = batch
            yield batch

    def __iter__(self):
        return iter(self.dataset)


def main():
    from data.dataset import Dataset
    Trainer = G.load_imitation_trainer()
    cfg, world = G.make_world()
    cfg.data_dir = "data"
    cfg.trainer.batch_size = BATCH
    cfg.trainer.max_timesteps = T_MAX
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
    stub = Stub(table, {iid: i for i, iid in enumerate(ids)})
    trainer = Trainer(cfg)
    distances = []
    rollout = trainer.do_rollout

    def recording_rollout(*a, **kw):
        info = rollout(*a, **kw)
        distances.extend(info["distances"])
        return info
    trainer.do_rollout = recording_rollout
    with contextlib.redirect_stdout(io.StringIO()):
        success_rate, eval_info = trainer.evaluate(Batches(ds, stub), world, stub, teacher)
    avg_distance = sum(distances) / len(distances)
    actions = np.full((N_INSTANCES, T_MAX), -1, dtype=np.int8)
    success = np.zeros(N_INSTANCES, dtype=np.int8)
    for i, iid in enumerate(ids):
        a = eval_info[iid]["actions"]
        actions[i, :len(a)] = a
        success[i] = eval_info[iid]["success"]
    n_act = (actions >= 0).sum(1)
    last = actions[np.arange(N_INSTANCES), n_act - 1]
    stops = int((last == STOP).sum())
    timeouts = int(((last != STOP) & (n_act == T_MAX)).sum())
    assert stops + timeouts == N_INSTANCES
    is_get = np.asarray([item["task"].goal_name == "get" for item in ds.data])
    counts = {"successes": int(success.sum()), "failures": int((success == 0).sum()),
              "failed get tasks with distance > 0": int(sum(d > 0 for d in distances)),
              "timeouts": timeouts, "STOP endings": stops}
    print(counts, "success rate", success_rate, "mean distance", avg_distance,
          "get tasks", int(is_get.sum()), len(distances))
    assert len(distances) == int(is_get.sum())
    for k, v in counts.items():
        assert v >= 10, (k, v)
    path = os.path.join(OUT, "imitation_evaluate.npz")
    np.savez_compressed(path, ids=np.asarray(ids), table=table, actions=actions, success=success,
                        success_rate=np.float64(success_rate), avg_distance=np.float64(avg_distance),
                        max_timesteps=np.int32(T_MAX), batch_size=np.int32(BATCH))
    print("imitation_evaluate.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
