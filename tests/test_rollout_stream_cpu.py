"""craft_rollout_stream on the CPU variant of the ABI (its loop of stream ticks into ring slots)
against the loop of craft_step_stream calls; what the shared checks refuse; that the rows the GPU
tests run exercise what they claim; and rollout.replay on the reference's demonstrations."""
import numpy as np
import pytest
import torch

from psketch_amd import _native as N
from psketch_amd import rollout
from tests import rollout_stream_refusal_cases as RC
from tests.refusal_cases import check_row, make_handles
from tests.rollout_stream_cases import LAUNCHES, ROW_IDS, ROWS, row_sims, run_rollout_against_steps
from tests.test_cpu_variant import cpu_sim
from tests.test_gpu_parity import set_states

N_TICKS = sum(LAUNCHES)


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("given", [True, False], ids=["given", "hashed"])
@pytest.mark.parametrize("ring", [1, 3, N_TICKS])
@pytest.mark.parametrize("fmt", ["f32", "bf16", "u8"])
def test_rollout_stream_cpu_equals_step_loop(fmt, ring, given, wrap):
    """n = 72, 30 ticks in launches of 7, 7, 7, 7, 2: every ring slot after every launch, then
    get_state() (spec included), stats() and check()."""
    row = ROWS[0][:5] + (fmt, ring, ROWS[0][7])
    specs, (a, b) = row_sims(row, cpu_sim, cpu_sim)
    # (what a run has to exercise is asserted on the GPU table's rows below)
    run_rollout_against_steps(a, b, specs, wrap, ring, given, coverage=False)


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_gpu_rows_meet_their_coverage(row, wrap):
    """Each row of the GPU table, as the GPU tests run it (given and hashed launches
    alternating), on the CPU variant: the step loop's outputs meet every coverage condition."""
    specs, (a, b) = row_sims(row, cpu_sim, cpu_sim)
    run_rollout_against_steps(a, b, specs, wrap, row[6], "alternate")


@pytest.fixture(scope="module")
def handles():
    return make_handles("cpu", names=RC.HANDLES)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_rollout_stream_refuses_cpu(handles, row):
    assert row.message.startswith("craft_rollout_stream: ")
    check_row(handles[row.handle], row)


def test_rollout_stream_no_ticks_is_a_no_op_cpu(handles):
    c = handles["begun"]
    before = c.sim.get_state()
    c.sim.rollout_stream(0)
    for k, v in c.sim.get_state().items():
        assert torch.equal(v, before[k]), k
    c.sim.check()


# ---- rollout.replay ------------------------------------------------------------------------------
def demo_inputs(golden, split="dev"):
    g = golden("devtest.npz")
    acts = g[f"{split}_actions"].astype(np.int32)
    seqs = [row[row >= 0] for row in acts]
    pos = g[f"{split}_pos"].astype(np.int32)
    count = len(seqs)
    specs = np.stack([g[f"{split}_world"], pos[:, 0], pos[:, 1], np.zeros(count), g[f"{split}_task"]], 1)
    return g[f"{split}_grids"], np.ascontiguousarray(specs.astype(np.int32)), seqs


def check_replay(sim, ref, specs, seqs, ticks_per_launch, n_pairs=50):
    """replay() of the demonstrations on `sim`; `ref` (n_pairs slots, any device) rebuilds the
    sampled states with set_state + transition + observe.  Returns the ReplayInfo."""
    count = len(seqs)
    length = np.asarray([len(s) for s in seqs])
    rng = np.random.RandomState(4)
    pe = rng.randint(0, count, size=n_pairs)
    ps = np.asarray([rng.randint(0, length[e]) for e in pe])
    want = {(int(e), int(s)): j for j, (e, s) in enumerate(zip(pe, ps))}
    rows = {}
    seen = np.zeros((count, length.max()), dtype=np.int32)
    chunks = []

    def on_chunk(obs, episode, step, action):
        assert obs.shape[:2] == episode.shape == step.shape == action.shape
        chunks.append(obs.shape[0])
        ep, st, ac = (x.cpu().numpy() for x in (episode, step, action))
        kk, ii = np.nonzero(ac >= 0)
        np.add.at(seen, (ep[kk, ii], st[kk, ii]), 1)
        for k, i in zip(kk, ii):
            e, s = int(ep[k, i]), int(st[k, i])
            assert ac[k, i] == seqs[e][s]
            if (e, s) in want:
                rows[(e, s)] = obs[k, i].cpu().clone()

    info = rollout.replay(sim, specs, seqs, ticks_per_launch=ticks_per_launch, on_chunk=on_chunk)
    assert chunks[0] == 1 and max(chunks[1:]) == ticks_per_launch and len(chunks) == info.launches + 1
    assert (info.success == 1).all()
    np.testing.assert_array_equal(info.length, length)
    # the rows with action >= 0: every recorded (state, action) pair exactly once
    assert int(seen.sum()) == int(length.sum())
    assert (seen[np.arange(seen.shape[1])[None] < length[:, None]] == 1).all()
    # the sampled rows against states rebuilt step by step
    sp = specs[pe]
    set_states(ref, sp[:, 0], np.concatenate([sp[:, 1:3], np.zeros((n_pairs, 1), np.int32)], 1),
               np.zeros((n_pairs, 1)), task=sp[:, 4])
    for t in range(int(ps.max())):
        a = np.asarray([seqs[e][t] if t < s else -1 for e, s in zip(pe, ps)], dtype=np.int32)
        ref.transition(torch.as_tensor(a, device=ref.device))
    obs = ref.empty_obs()
    ref.observe(obs=obs)
    ref.check()
    for (e, s), j in want.items():
        assert torch.equal(rows[(e, s)], obs[j].cpu()), (e, s)
    return info


def test_replay_reference_demonstrations_cpu(golden):
    grids, specs, seqs = demo_inputs(golden)
    sim = cpu_sim("craft_medium", 64, grids)
    check_replay(sim, cpu_sim("craft_medium", 50, grids), specs, seqs, 32)


def test_replay_refuses_bad_sequences(golden):
    grids, specs, seqs = demo_inputs(golden)
    sim = cpu_sim("craft_medium", 8, grids)
    specs, seqs = specs[:20], seqs[:20]
    early = list(seqs)
    early[3] = np.asarray([N.UP, N.STOP, N.UP, N.STOP])
    with pytest.raises(ValueError, match="episode 3"):
        rollout.replay(sim, specs, early)
    short = list(seqs)
    short[5] = np.asarray([N.UP, N.DOWN])
    short[7] = np.asarray([N.UP])
    with pytest.raises(ValueError, match="episode 5"):
        rollout.replay(sim, specs, short)
    bad = list(seqs)
    bad[2] = np.asarray([6, N.STOP])
    with pytest.raises(ValueError, match="episode 2"):
        rollout.replay(sim, specs, bad)
    rollout.replay(sim, specs, seqs)                 # the sequences as recorded pass
