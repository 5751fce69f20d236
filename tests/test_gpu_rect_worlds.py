"""The HIP kernels on worlds with WIDTH != HEIGHT (tests/helpers.py RECT_SHAPES): every entry
point against the oracle where the oracle has the operation (and against the reference's own
results, tests/golden/rect_worlds.npz, for the slot-list entry points), else against the CPU variant
of the ABI, which tests/test_rect_worlds.py pins on the same shapes.  Small batches (200 envs: a
partial last tile for 16-, 32- and 64-env tiles; 300 for the two-tile tick), at most 48 ticks."""
import numpy as np
import pytest
import torch

from tests.helpers import RECT_FIXTURE_TAGS, RECT_SHAPES, rect_world
from tests.rect_cases import (FORMATS, host, make_sim, oracle_labels, rect_case, run_lockstep, run_rollout,
                              run_step_teach)
from tests.test_gpu_step_lang import lang_lockstep
from tests.test_gpu_step_stream import stream_lockstep
from tests.test_rect_worlds import (check_distances_vs_oracle, check_kats, check_pool_generate, check_teach_rollout,
                                    teach_reference)

pytestmark = pytest.mark.gpu

TAGS = list(RECT_SHAPES)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rect_worlds.npz")


# ---- the tile kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_step_lockstep_vs_oracle(oracle_mod, tag):
    """craft_step every tick against the oracle (45 ticks: timeouts and restarts), formats f32 /
    bf16 / u8 and tiles default / 16 / 64 cycled over the shapes; craft_teacher of every env at
    tick 20 and at the end (15x16 and 16x15 are the largest worlds it accepts)."""
    i = TAGS.index(tag)
    case = rect_case(oracle_mod, tag)
    sim = make_sim(case, 0)
    tile = (0, 16, 64)[(i // 3 + i) % 3]
    if tile:
        sim.tune(tile_envs=tile, obs_store=2)
        assert sim.tile_shape()[0] == tile
    run_lockstep(sim, case, oracle_mod, fmt=FORMATS[i % 3], teacher_at=(20, 44))


# ---- craft_rollout ------------------------------------------------------------------------------
# tile: craft_sim_tune's tile_envs; chunk / threads: craft_sim_tune_rollout's; R: the ring (0 = the
# launch's 12 ticks); split: the split-producer kernel, where the row fixes it
ROLLOUT_ROWS = [
    ("r7x13", 0, 0, 0, 0, "f32", True),        # the default shape: the split-producer kernel
    ("r16x15", 0, 0, 0, 0, "bf16", True),
    ("r13x7", 0, 2, 0, 3, "f32", None),        # tiles handed between workgroups, a ring shorter than a launch
    ("r16x6", 0, 0, 256, 0, "u8", False),      # rollout_kernel
    ("r16x6", 0, -1, 0, 0, "f32", None),       # the continuous pipeline
    ("r10x16", 0, 0, 0, 0, "bf16", None),
    ("r5x16", 0, 0, 0, 0, "f32", None),        # the window is larger than the world
    ("r16x5", 0, 0, 0, 0, "u8", None),
    # tile_envs 64 asked for: two staged 7x7 observation buffers of 64 envs (267 KB) exceed a
    # workgroup's LDS, so the library runs 32-env tiles and reports them
    ("r15x16", 64, 0, 0, 0, "f32", None)]


@pytest.mark.parametrize("tag,tile,chunk,threads,R,fmt,split", ROLLOUT_ROWS,
                         ids=[f"{r[0]}-tile{r[1]}-chunk{r[2]}-threads{r[3]}-ring{r[4]}" for r in ROLLOUT_ROWS])
def test_rollout_vs_oracle(oracle_mod, tag, tile, chunk, threads, R, fmt, split):
    """Four craft_rollout launches of 12 ticks against the oracle's per-tick results."""
    case = rect_case(oracle_mod, tag)
    sim = make_sim(case, 0)
    if tile:
        sim.tune(tile_envs=tile, obs_store=2)
    sim.tune_rollout(chunk, threads)
    shape = sim.rollout_shape()
    assert not threads or shape[1] == threads, shape
    assert not tile or shape[0] == (32 if case.window == 7 else tile), shape
    assert split is None or shape[2] == split, shape
    run_rollout(sim, case, oracle_mod, fmt=fmt, launches=4, K=12, R=R or None)


# ---- craft_step_teach ---------------------------------------------------------------------------
# kernel / lanes: craft_sim_tune_teach's (kernel 2: the two-tile kernel, 300 envs); tile:
# craft_sim_tune's tile_envs; the table is forced on and off alternately (1, 2)
TEACH_ROWS = [
    ("r7x13", 300, 2, 0, 0),
    ("r16x15", 300, 2, 0, 0),
    ("r6x16", 200, 1, 4, 0),
    ("r10x16", 200, 0, 2, 0),
    ("r12x16", 200, 0, 4, 64),
    ("r16x12", 200, 0, 0, 0),
    ("r15x16", 200, 0, 0, 0),
    ("r13x7", 200, 0, 1, 0)]


@pytest.mark.parametrize("tag,n,kernel,lanes,tile", TEACH_ROWS,
                         ids=[f"{r[0]}-kernel{r[2]}-lanes{r[3]}-tile{r[4]}" for r in TEACH_ROWS])
def test_step_teach_vs_oracle(oracle_mod, tag, n, kernel, lanes, tile):
    table = 1 + [r[0] for r in TEACH_ROWS].index(tag) % 2
    case = rect_case(oracle_mod, tag, n=n)
    sim = make_sim(case, 0)
    sim.tune_teach(kernel, lanes, table)
    if tile:
        sim.tune(tile_envs=tile, obs_store=2)
    name, envs_per, _ = sim.step_shape(teach=True)
    assert (name, envs_per) == (("tick2_kernel", 128) if kernel == 2 else ("tile_kernel", tile or envs_per))
    run_step_teach(sim, case, oracle_mod, T=30)


# ---- craft_rollout_teach ------------------------------------------------------------------------
@pytest.mark.parametrize("table", [1, 2], ids=["table_on", "table_off"])
@pytest.mark.parametrize("tag,mode", [("r7x13", "policy"), ("r16x6", "label"), ("r10x16", "bc"),
                                      ("r12x16", "label"), ("r15x16", "policy"), ("r5x16", "label")])
def test_rollout_teach_vs_oracle(oracle_mod, tag, mode, table):
    """Three launches of 16 ticks chaining label_in against rollout_oracle.teach_rollout (computed
    once per row): labels, action_record, done, success, observations, states."""
    case, o, a, refs = teach_reference(oracle_mod, tag, mode, n=200, launches=3, K=16, want_obs=True)
    sim = make_sim(case, 0)
    sim.tune_teach(0, 0, table)
    check_teach_rollout(sim, case, a, refs, K=16)


# ---- craft_step_lang, craft_step_stream ---------------------------------------------------------
@pytest.mark.parametrize("tag,n", [("r13x7", 72), ("r6x16", 200)])
def test_step_lang_hip_equals_cpu_variant(tag, n):
    W, H, window, prims = RECT_SHAPES[tag]
    lang_lockstep(rect_world(W, H, window, prims), W, n, 0, 0, True, "f32", 0, H=H)


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("tag,n", [("r13x7", 72), ("r6x16", 200)])
def test_step_stream_hip_equals_cpu_variant(tag, n, wrap):
    W, H, window, prims = RECT_SHAPES[tag]
    stream_lockstep(rect_world(W, H, window, prims), W, n, 0, 0, True, "f32", 0, wrap, H=H)


# ---- craft_pool_generate, the teacher table over its rows ---------------------------------------
@pytest.mark.parametrize("tag", ["r7x13", "r16x5", "r6x16", "r15x16"])
def test_pool_generate_and_table_labels_vs_oracle(oracle_mod, tag):
    check_generated_pool_labels(oracle_mod, tag, 0)


def check_generated_pool_labels(oracle_mod, tag, device):
    """64 generated scenarios against the oracle's splitmix stream; then, with the teacher table
    forced on, the labels of envs on the generated rows (craft_teacher and 8 ticks of
    craft_step_teach) against oracle.teacher: the table's (slot*4+dir)*C + x*H + y addressing."""
    count = 64
    sim, grids, init = check_pool_generate(oracle_mod, tag, device, count)
    sim.tune_teach(0, 0, 1)
    tasks = np.asarray([t.id for t in sim.task_manager.dataset_tasks()], dtype=np.int32)
    ids = np.arange(count)
    specs = ((3 + ids).astype(np.int32), init[:, 0], init[:, 1], (ids % 4).astype(np.int32), tasks[ids % len(tasks)])
    sim.reset(*specs)
    o = oracle_mod.Oracle(sim.config, np.concatenate([np.zeros((3, grids.shape[1]), np.uint8), grids]))
    envs = o.init_envs(*specs)
    seen = set()
    lab = torch.empty(count, dtype=torch.int32, device=sim.device)
    got, _ = sim.teacher()
    for t in range(9):
        want = oracle_labels(o, envs)
        np.testing.assert_array_equal(host(got), want, err_msg=f"t={t}")
        seen |= set(want.tolist())
        if t == 8:
            break
        sim.step(seed=9, tick=t, labels=lab)
        rc, *_ = o.batch_tick(envs, 0, None, 9, t, True, False)
        assert rc == 0
        got = lab
    assert seen >= {0, 1, 2, 3} and -2 not in seen
    sim.check()


# ---- craft_rollout_distances --------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["r13x7", "r15x16"])
def test_rollout_distances_vs_oracle_and_cpu_variant(oracle_mod, tag):
    g = check_distances_vs_oracle(oracle_mod, tag, 0)
    c = check_distances_vs_oracle(oracle_mod, tag, "cpu")
    for x, y in zip(g, c):
        np.testing.assert_array_equal(x, y)


# ---- craft_set_state / craft_observe / craft_transition / craft_get_state on slot lists ---------
@pytest.mark.parametrize("tag", RECT_FIXTURE_TAGS)
def test_random_step_kats(fx, tag):
    check_kats(fx, tag, 0)
