"""The HIP kernels on cookbooks up to the ABI's limits (tests/cookbook_cases.py: 32 kinds, 16
recipes of up to 4 ingredients, 64 tasks of up to 4 subtasks; 22 and 12 kinds, whose observation
rows are odd): every entry point against the oracle where the oracle has the operation (and against
the reference's own results, tests/golden/cookbook_limits.npz), else against the CPU variant of the
ABI, which tests/test_cookbook_limits.py pins on the same cases.  Everything is exact.  35 and 70
envs (a 32-env tile and 3, a 64-env tile and 6) for the one-tick entry points; the K-tick entry
points, whose observation ring slots must start on 16-byte boundaries, take 36 / 68 (f32), 40 / 72
(bf16) and 48 / 80 (u8) envs of these odd rows."""
import numpy as np
import pytest

import tests.episode_summary_cases as S
from tests.cookbook_cases import COOKBOOKS, cookbook_case
from tests.rect_cases import make_sim
from tests.test_cookbook_limits import (LOCKSTEP_ROWS, QUEUE_KINDS, check_create_refusals, check_distances,
                                        check_fixture_kats, check_fixture_rollout, check_fixture_teacher,
                                        check_pool_generate, check_recipes_need_every_ingredient, check_summary,
                                        check_tile_that_does_not_fit,
                                        check_top_kind_saturates, lockstep, rollout, rollout_teach, run_queue,
                                        step_teach)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden):
    return golden("cookbook_limits.npz")


# ---- craft_step / craft_step_ex -----------------------------------------------------------------
@pytest.mark.parametrize("name,world,fmt", LOCKSTEP_ROWS)
def test_step_lockstep_vs_oracle(oracle_mod, name, world, fmt):
    """36 ticks against the oracle, 35 and 70 envs and the tiles default / 16 / 64 cycled over the
    rows (64 where it fits: not at 7x7 windows with 32 kinds); craft_teacher of every env at three
    ticks.  The fp32 rows end their tail tile off a 16-byte boundary (stream_obs's scalar tail)."""
    i = LOCKSTEP_ROWS.index((name, world, fmt))
    tile = (0, 16, 64)[i % 3]
    if tile == 64 and name == "limits" and world == "w7":
        tile = 16
    sim = lockstep(oracle_mod, 0, name, world, fmt, n=70 if i % 2 else 35, tile=tile)
    assert not tile or sim.tile_shape()[0] == tile


# ---- craft_rollout ------------------------------------------------------------------------------
# cookbook, world, format, n (0 / 1: index into RING_N[format]; else the env count), craft_sim_tune's tile, craft_sim_tune_rollout's
# threads and chunk, ring (None: the launch's 12 ticks), the shape craft_sim_rollout_shape reports
ROLLOUT_ROWS = [
    ("limits", "w3", "f32", 0, 0, 0, 0, None, (32, 512, True)),          # the default: the split-producer kernel
    ("even", "w3", "bf16", 1, 0, 0, 0, None, (32, 512, True)),
    ("limits", "w3", "u8", 1, 0, 0, 0, 5, (32, 512, True)),              # a ring shorter than the launch
    ("limits", "w3", "bf16", 0, 16, 128, 0, None, (16, 128, False)),
    ("even", "w3", "f32", 1, 16, 128, 0, 5, (16, 128, False)),
    ("limits", "w3", "f32", 1, 64, 512, 0, None, (64, 512, False)),
    ("even", "w3", "u8", 0, 64, 512, 0, None, (64, 512, False)),
    ("limits", "w3", "f32", 1, 32, 512, -1, None, (32, 512, True)),      # the continuous pipeline
    ("even", "w3", "bf16", 0, 32, 512, -1, None, (32, 512, True)),
    ("limits", "w3", "u8", 0, 0, 0, 2, None, (32, 512, True)),           # tiles handed between workgroups
    ("even", "w3", "f32", 0, 0, 0, 2, 5, (32, 512, True)),
    # 32 kinds: two staged buffers of 64 envs at 5x5 (209 KB) and of 32 envs at 7x7 (203 KB) exceed a
    # workgroup's LDS, so the library runs the largest tile that fits and reports it
    ("limits", "w5", "f32", 1, 64, 0, 0, None, (32, 256, False)),
    ("limits", "w7", "f32", 1, 32, 0, 0, None, (16, 256, False)),
    ("limits", "w7", "bf16", 0, 0, 0, 0, None, (16, 256, False)),
    ("even", "w7", "u8", 1, 32, 0, 0, 5, (32, 256, False)),              # 22 kinds: 32 envs fit (140 KB)
    ("even", "w5", "bf16", 1, 0, 0, 0, None, (32, 256, False)),
    # a ring of one slot, which has no alignment rule: 35 envs, so the fp32 tail tile (3 envs, or all 35
    # of one 64-env tile) ends off a 16-byte boundary and stream_obs's scalar tail runs in the K-tick kernels
    ("limits", "w3", "f32", 35, 0, 0, 0, 1, (32, 512, True)),
    ("even", "w3", "f32", 35, 0, 0, 0, 1, (32, 512, True)),
    ("limits", "w3", "f32", 35, 16, 128, 0, 1, (16, 128, False)),
    ("even", "w3", "f32", 35, 64, 512, 0, 1, (64, 512, False)),
    ("limits", "w7", "f32", 35, 0, 0, 0, 1, (16, 256, False))]


@pytest.mark.parametrize("name,world,fmt,n,tile,threads,chunk,R,shape", ROLLOUT_ROWS,
                         ids=[f"{r[0]}-{r[1]}-{r[2]}-n{r[3]}-tile{r[4]}-threads{r[5]}-chunk{r[6]}-ring{r[7]}"
                              for r in ROLLOUT_ROWS])
def test_rollout_vs_oracle(oracle_mod, name, world, fmt, n, tile, threads, chunk, R, shape):
    """Three craft_rollout launches of 12 ticks against the oracle's per-tick results."""
    rollout(oracle_mod, 0, name, world, fmt, n=n if n < 2 else 0, tile=tile, threads=threads, chunk=chunk, R=R,
            shape=shape, envs=n if n >= 2 else None)


# ---- craft_step_teach ---------------------------------------------------------------------------
# world, n, craft_sim_tune_teach's kernel (2: the two-tile kernel, 128-env workgroups), lanes and
# table (1 on, 2 off), the (kernel, envs per workgroup) craft_sim_step_shape reports
TEACH_ROWS = [("w3", 70, 1, 1, 1, ("tile_kernel", 64)), ("w3", 70, 1, 2, 2, ("tile_kernel", 64)),
              ("w3", 70, 1, 4, 1, ("tile_kernel", 64)), ("w3", 140, 2, 2, 2, ("tick2_kernel", 128)),
              ("w3", 140, 2, 4, 1, ("tick2_kernel", 128)), ("w3", 35, 0, 0, 0, ("tile_kernel", 64)),
              ("w5", 70, 1, 4, 2, ("tile_kernel", 32)), ("w7", 35, 1, 2, 1, ("tile_kernel", 32))]


@pytest.mark.parametrize("world,n,kernel,lanes,table,shape", TEACH_ROWS,
                         ids=[f"{r[0]}-{r[1]}-kernel{r[2]}-lanes{r[3]}-table{r[4]}" for r in TEACH_ROWS])
def test_step_teach_vs_oracle(oracle_mod, world, n, kernel, lanes, table, shape):
    step_teach(oracle_mod, 0, "limits", world, n=n, kernel=kernel, lanes=lanes, table=table, shape=shape)


# ---- craft_rollout_teach ------------------------------------------------------------------------
@pytest.mark.parametrize("table", [1, 2], ids=["table_on", "table_off"])
@pytest.mark.parametrize("mode", ["policy", "bc", "label"])
@pytest.mark.parametrize("world", ["w3", "w7"])
def test_rollout_teach_vs_oracle(oracle_mod, world, mode, table):
    rollout_teach(oracle_mod, 0, "limits", world, mode, table=table)


# ---- the reference's own results: slot lists, craft_teacher with path_len_out, the hashed rollout
@pytest.mark.parametrize("name", COOKBOOKS)
def test_fixture_kats_and_rollout(fx, name):
    check_fixture_kats(fx, name, 0)
    check_fixture_rollout(fx, name, 0)


@pytest.mark.parametrize("name", COOKBOOKS)
def test_fixture_teacher(fx, name):
    check_fixture_teacher(fx, name, 0)


# ---- craft_rollout_distances, craft_pool_generate -----------------------------------------------
def test_rollout_distances_vs_oracle_and_cpu_variant(oracle_mod):
    g = check_distances(oracle_mod, "limits", "w3", 0)
    c = check_distances(oracle_mod, "limits", "w3", "cpu")
    for x, y in zip(g, c):
        np.testing.assert_array_equal(x, y)


def test_pool_generate_vs_oracle(oracle_mod):
    check_pool_generate(oracle_mod, "limits", "w3", 0)


# ---- the episode queue: HIP against the CPU variant ---------------------------------------------
# every runner on limits and even; the K-tick launches also on limits at 7x7 windows and, with a
# ring of one slot and 35 envs (the fp32 scalar tail in their kernels), at 3x3
K_TICK = ("rollout_stream", "rollout_teach_stream", "rollout_replay")
QUEUE_ROWS = [(k, n, "w3", 3) for n in ("limits", "even") for k in QUEUE_KINDS] + \
             [(k, "limits", "w7", 3) for k in K_TICK] + [(k, "limits", "w3", 1) for k in K_TICK]


@pytest.mark.parametrize("kind,name,world,ring", QUEUE_ROWS)
def test_queue_hip_equals_cpu_variant(kind, name, world, ring):
    """The shared runners on a cookbook's queue: HIP against the CPU variant tick by tick for the
    one-tick entry points; for the K-tick ones HIP against HIP's step_stream loop and the CPU
    variant's K-tick launch.
    The 7x7 rows: two staged 32-env buffers of 32 kinds (230 KB) exceed a workgroup's 160 KiB, so
    craft_rollout_stream and craft_rollout_replay must run 16-env tiles there.  No entry point
    reports their tile, so that is inferred, not asserted: the launcher refuses a carve past 160 KiB
    (CRAFT_EHIP), hence a launch that succeeds ran 16-env tiles; the results are then compared."""
    run_queue(kind, name, world, (0, "cpu") if kind in ("stream", "lang_stream") else (0, 0, "cpu"), ring=ring)


@pytest.mark.parametrize("name", ["limits", "even"])
def test_summary_vs_references_and_cpu_variant(oracle_mod, name):
    """craft_episode_summary with distance_out: against the host loop's copy and the oracle, then
    the CPU variant on the same records, the teacher table on and off."""
    case, specs, hr, got = check_summary(oracle_mod, 0, name)
    cpu = S.make_sim(case.params, 35, case.pool, got["actions"].shape[1], "cpu", **case.kw)
    S.begin(cpu, specs)
    want = S.summarise(cpu, S.on_device(hr, cpu), len(specs))
    cpu.check()
    for k in S.OUTPUTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    sim = S.make_sim(case.params, 35, case.pool, got["actions"].shape[1], 0, **case.kw)
    S.begin(sim, specs)
    sim.tune_teach(table=2)
    off = S.summarise(sim, S.on_device(hr, sim), len(specs))
    sim.check()
    for k in S.OUTPUTS:
        np.testing.assert_array_equal(off[k], want[k], err_msg=f"table off: {k}")


# ---- edges --------------------------------------------------------------------------------------
def test_top_kind_saturates(oracle_mod):
    check_top_kind_saturates(oracle_mod, 0)


def test_recipes_need_every_ingredient(oracle_mod):
    check_recipes_need_every_ingredient(oracle_mod, 0)


def test_tile_that_does_not_fit(oracle_mod):
    check_tile_that_does_not_fit(oracle_mod, 0)


def test_teacher_tick_picks_a_tile_that_fits(oracle_mod):
    """craft_sim_tune(16) at 7x7 windows: the teacher's one-tile kernel, which takes 64-env tiles
    of its own then, runs 32-env tiles where 64 envs of 32 kinds do not fit."""
    case = cookbook_case(oracle_mod, "limits", "w7", n=35)
    sim = make_sim(case, 0, **case.kw)
    sim.tune(tile_envs=16, obs_store=2)
    assert sim.step_shape(teach=True)[:2] == ("tile_kernel", 32)
    case = cookbook_case(oracle_mod, "even", "w7", n=35)
    sim = make_sim(case, 0, **case.kw)
    sim.tune(tile_envs=16, obs_store=2)
    assert sim.step_shape(teach=True)[:2] == ("tile_kernel", 64)          # 22 kinds: 64 envs fit (157 KB)


def test_create_refuses_one_past_each_limit(capfd):
    check_create_refusals(False, capfd)
