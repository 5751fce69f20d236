"""craft_episode_summary on the HIP library: the shared cases of tests/episode_summary_cases.py
against the copy of the host loop it replaces and against the oracle, the HIP library against the
CPU variant on identical records (with the teacher table on and off, per launch with carry, and
above 16,384 entries, where the distance kernel runs 2 lanes per entry instead of 4), the refusals
of tests/episode_summary_refusal_cases.py and the HIP library's own refusal under stream capture."""
import numpy as np
import pytest
import torch

from psketch_amd import _native as N
from tests import episode_summary_cases as C
from tests import episode_summary_refusal_cases as RC
from tests.refusal_cases import check_row, make_handles
from tests.stream_cases import T_MAX, queue_inputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lang", [False, True], ids=["step_stream", "step_lang_stream"])
def test_dev_split_table_on_and_off(golden, oracle_mod, lang):
    C.check_dev_split(golden, oracle_mod, 0, lang)


@pytest.mark.parametrize("n,rows,ticks", [(70, None, None), (20, 7, None), (70, None, 1)],
                         ids=["70_slots", "20_slots_7_rows", "one_tick"])
def test_slot_counts(oracle_mod, n, rows, ticks):
    C.check_slot_counts(oracle_mod, 0, n, rows=rows, ticks=ticks)


def test_every_slot_stops_every_tick(oracle_mod):
    C.check_every_slot_stops_every_tick(oracle_mod, 0)


def test_records_without_an_end():
    C.check_no_end(0)


@pytest.mark.parametrize("mode", ["hashed", "label"])
def test_chunks_with_carry(oracle_mod, mode):
    C.check_chunks(oracle_mod, 0, mode)


@pytest.mark.parametrize("tag", [C.RECT_SMALLEST, C.RECT_LARGEST])
def test_rectangular_worlds(oracle_mod, tag):
    C.check_rect(oracle_mod, 0, tag)


def test_flags_and_latches(golden, oracle_mod):
    C.check_flags(golden, oracle_mod, 0)


def test_handle_left_alone():
    C.check_handle_left_alone(0)


@pytest.mark.parametrize("lang", [False, True], ids=["evaluate", "language_evaluate"])
def test_evaluate_leaves_the_handle(golden, lang):
    C.check_evaluate_leaves_the_handle(golden, 0, lang)


def test_replay_reports_distances(golden, oracle_mod):
    C.check_replay_distances(golden, oracle_mod, 0)


# ---- the HIP library against the CPU variant on identical records --------------------------------
def cpu_twin(world, n, pool, specs, T):
    """A CPU-variant handle with the same pool and queue as the handle under test."""
    cpu = C.make_sim(world, n, pool, T, "cpu")
    C.begin(cpu, specs)
    return cpu


def assert_hip_equals_cpu(sim, cpu, r, count, what):
    """One call over the device records r on the HIP library, table on and off, and over their
    host copy on the CPU variant: every output equal.  Returns the outputs."""
    hr = C.on_device(C.host(r), cpu)
    want = C.summarise(cpu, hr, count)
    cpu.check()
    for table in (0, 2):
        sim.tune_teach(table=table)
        got = C.summarise(sim, r, count)
        sim.check()
        for k in C.OUTPUTS:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}, table {table}: {k}")
    sim.tune_teach(table=0)
    return want


@pytest.mark.parametrize("lang", [False, True], ids=["step_stream", "step_lang_stream"])
def test_hip_equals_cpu_variant_on_the_dev_split(golden, lang):
    pool, specs, sim = C.dev_setup(golden, 0)
    r = C.stream_pass(sim, specs, C.hash_policy(sim), lang=lang)
    out = assert_hip_equals_cpu(sim, cpu_twin("craft_medium", sim.n_envs, pool, specs, C.DEV_T), r, len(specs), "dev")
    assert (out["success"] != -2).all() and (out["distance"] > 0).any()


def test_hip_equals_cpu_variant_per_launch_with_carry():
    """The label-mode launches of the chunk case summarised launch by launch on both libraries:
    the outputs and the run carry are equal after every launch."""
    n, T, K = 40, 4, 5
    pool, specs = queue_inputs(C.W12, 12, n)
    count = len(specs)
    sim = C.make_sim(C.W12, n, pool, T, 0)
    chunks = C.chunk_records(sim, specs, "label", K=K)
    cpu = cpu_twin(C.W12, n, pool, specs, T)
    run_g, run_c = torch.zeros(n, dtype=torch.int32, device=sim.device), torch.zeros(n, dtype=torch.int32)
    outs_g, outs_c = {}, {}
    for l, r in enumerate(chunks):
        hr = C.on_device(C.host(r), cpu)
        g = sim.episode_summary(r["ended"], r["pose"], r["succ"], action_record=r["rec"], count=count, run=run_g,
                                episode_now=r["now"][K - 1], **outs_g)
        c = cpu.episode_summary(hr["ended"], hr["pose"], hr["succ"], action_record=hr["rec"], count=count, run=run_c,
                                episode_now=hr["now"][K - 1], **outs_c)
        outs_g, outs_c = ({k + "_out": v for k, v in o.items()} for o in (g, c))
        for k in C.OUTPUTS:
            np.testing.assert_array_equal(g[k].cpu().numpy(), c[k].numpy(), err_msg=f"launch {l}: {k}")
        np.testing.assert_array_equal(run_g.cpu().numpy(), run_c.numpy(), err_msg=f"launch {l}: run")
    sim.check()
    cpu.check()
    assert (run_c > 0).any()


def test_two_lanes_per_entry_above_16384_entries(oracle_mod):
    """16,384 + 130 entries on 4,096 slots, 30 ticks of craft_rollout_stream with hashed actions
    in one launch: the distance kernel runs 2 lanes per entry.  Against the CPU variant on the
    same records, table on and off, and a sample of the failed get episodes against the oracle."""
    n, ticks, seed = 4096, 30, 4
    pool, specs = queue_inputs(C.W12, 12, n)
    specs = np.ascontiguousarray(np.tile(specs, (2, 1))[:16384 + 130])
    count = len(specs)
    sim = C.make_sim(C.W12, n, pool, T_MAX, 0)
    C.begin(sim, specs)
    i32 = dict(dtype=torch.int32, device=sim.device)
    r = {k: torch.empty((ticks, n), **i32) for k in ("ended", "pose", "now")}
    r["succ"] = torch.empty((ticks, n), dtype=torch.int8, device=sim.device)
    sim.rollout_stream(ticks, seed=seed, success=r["succ"], episode_end=r["ended"], end_pose=r["pose"],
                       episode_now=r["now"])
    sim.check()
    now = r["now"].cpu().numpy()
    running = np.concatenate([np.ones((1, n), bool), now[:-1] >= 0])
    rec = np.stack([C.hash_actions(seed, np.arange(n), t) for t in range(ticks)]).astype(np.int32)
    r["rec"] = torch.as_tensor(np.where(running, rec, -1).astype(np.int32)).to(sim.device)
    out = assert_hip_equals_cpu(sim, cpu_twin(C.W12, n, pool, specs, T_MAX), r, count, "16514 entries")
    assert (out["success"] != -2).all(), "the pass did not finish every entry"
    cfg = sim.config
    failed = np.nonzero((out["distance"] != 0) & (out["distance"] != -1) & (out["success"] == 0))[0]
    assert len(failed) > 1000
    sample = failed[np.random.RandomState(1).choice(len(failed), 200, replace=False)]
    pose = np.stack(C.pose_xyd(out["end_pose"]), 1)
    want = C.oracle_distances(oracle_mod, cfg, pool, specs[sample], out["success"][sample], pose[sample])
    np.testing.assert_array_equal(out["distance"][sample], want)


# ---- refusals ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles():
    return make_handles(0, names=RC.HANDLES)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_episode_summary_refuses_hip(handles, row):
    check_row(handles[row.handle], row)


def test_episode_summary_accepts_hip(handles):
    RC.check_accepts(handles["queued"])


def test_episode_summary_capture_right_after_pool_load():
    """The HIP library's own refusal: a call with distance_out captured straight after load_pool,
    while the new rows wait for their teacher-table entries, is refused and leaves the handle
    usable; without distance_out the table is not read and the capture goes through."""
    n = 72
    pool, specs = queue_inputs(C.W12, 12, n)
    sim = C.make_sim(C.W12, n, pool, T_MAX, 0)
    C.begin(sim, specs)
    i32 = dict(dtype=torch.int32, device=sim.device)
    r = {"ended": torch.full((2, n), -1, **i32), "pose": torch.full((2, n), -1, **i32),
         "succ": torch.full((2, n), -1, dtype=torch.int8, device=sim.device)}
    r["ended"][1] = torch.arange(n, **i32)
    r["pose"][1] = torch.as_tensor(specs[:n, 1] | (specs[:n, 2] << 8) | (specs[:n, 3] << 16), **i32)
    r["succ"][1] = 0
    outs = {k: v for k, v in sim.episode_summary(r["ended"], r["pose"], r["succ"], distances=False).items()
            if v is not None}
    outs = {k + "_out": v for k, v in outs.items()}
    dist = torch.full((len(specs),), -1, **i32)
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    sim.load_pool(pool)                      # the rows wait for their table entries again
    with pytest.raises(N.CraftError, match="sync_table"):
        with torch.cuda.stream(st):
            with torch.cuda.graph(g, stream=st):
                sim.episode_summary(r["ended"], r["pose"], r["succ"], distance_out=dist, **outs)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g2, stream=st):
            sim.episode_summary(r["ended"], r["pose"], r["succ"], distances=False, **outs)
    outs["length_out"].zero_()
    g2.replay()
    torch.cuda.synchronize()
    assert (outs["length_out"][:n] == 2).all() and (outs["length_out"][n:] == 0).all()
    eager = sim.episode_summary(r["ended"], r["pose"], r["succ"], distance_out=dist, **outs)
    sim.check()
    cpu = cpu_twin(C.W12, n, pool, specs, T_MAX)
    want = C.summarise(cpu, C.on_device(C.host(r), cpu), len(specs))
    np.testing.assert_array_equal(eager["distance"].cpu().numpy(), want["distance"])
