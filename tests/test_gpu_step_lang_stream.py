"""craft_step_lang_stream on the card (the tile kernel's MODE_LANG_STREAM, craft_tile.h): in
lockstep with the CPU variant of the same ABI (itself checked by tests/test_lang_stream_cpu.py),
the end-on-a-grab known-answer test, against the composition of the existing HIP entry points, as
one captured graph, its refusals, and language_rollout.evaluate against do_language_rollout and
the reference's evaluate of the language trainers."""
import numpy as np
import pytest
import torch

from tests.helpers import RECT_SHAPES, make_tables, rect_world, row_ids
from tests.lang_stream_cases import (LANG_STREAM_OUTPUTS, check_end_on_a_grab, check_lang_against_composition,
                                     check_turn_away_times_out, grab_queue, lang_stream_buffers, run_lang_lockstep,
                                     turned_away_faces_other)
from tests.lang_stream_refusal_cases import HANDLES, ROWS
from tests.language_evaluate_cases import check_evaluate_equals_language_rollout, check_evaluate_equals_reference
from tests.refusal_cases import check_row, make_handles
from tests.stream_cases import T_MAX, queue_inputs
from tests.test_cpu_variant import cpu_sim
from tests.test_gpu_parity import sim_with_pool
from tests.test_gpu_step_stream import STREAM_ROWS, W12

pytestmark = pytest.mark.gpu

R7x13 = rect_world(*RECT_SHAPES["r7x13"])
# STREAM_ROWS' shapes (tests/test_gpu_step_stream.py says what each covers), and a WIDTH != HEIGHT
# world, 7 x 13, with the teacher and without: (world, W, n, lanes, table, teach, fmt, tile, H)
LANG_STREAM_ROWS = [r + (None,) for r in STREAM_ROWS] + [
    (R7x13, 7, 70, 0, 0, True, "f32", 0, 13),
    (R7x13, 7, 70, 2, 2, False, "bf16", 0, 13)]


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("world,W,n,lanes,table,teach,fmt,tile,H", LANG_STREAM_ROWS,
                         ids=row_ids(LANG_STREAM_ROWS, 7, ("tile", "H")))
def test_step_lang_stream_hip_equals_cpu_variant(world, W, n, lanes, table, teach, fmt, tile, H, wrap):
    pool, specs = queue_inputs(world, W, n, H=H)
    g, c = sim_with_pool(world, n, pool, max_timesteps=T_MAX), cpu_sim(world, n, pool, max_timesteps=T_MAX)
    g.tune_teach(1, lanes, table)
    if tile:
        g.tune(tile_envs=tile, obs_store=2)      # (2: the store policy of an untuned handle)
    for s in (g, c):
        s.set_obs_format(fmt)
    run_lang_lockstep(g, c, specs, wrap, teach=teach)


@pytest.mark.parametrize("teach", [True, False], ids=["labels", "no_labels"])
def test_end_on_a_grab(teach):
    n = 70
    pool, specs, _ = grab_queue(W12, 12, 12, n)
    a, ref = sim_with_pool(W12, n, pool, max_timesteps=1), cpu_sim(W12, n, pool, max_timesteps=1)
    check_end_on_a_grab(a, ref, pool, specs, teach=teach)
    a.check()


def test_turn_away_then_use_times_out():
    n = 70
    pool, specs, _ = grab_queue(W12, 12, 12, n)
    cfg = make_tables(W12, 2)[3]
    keep = np.asarray([turned_away_faces_other(pool, cfg, 12, 12, s) for s in specs])
    check_turn_away_times_out(sim_with_pool(W12, n, pool, max_timesteps=2), np.ascontiguousarray(specs[keep][:n]))


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
def test_step_lang_stream_equals_step_lang_set_state_observe_teacher(wrap):
    n = 200
    pool, specs = queue_inputs(W12, 12, n)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    check_lang_against_composition(a, b, specs, wrap)


def test_step_lang_stream_linear_graph():
    """Four step_lang_stream launches captured as one linear graph (no parallel branches), reading
    an actions buffer updated in place, replayed three times: equal to twelve eager ticks."""
    n = 200
    pool, specs = queue_inputs(W12, 12, n)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes()
        s.sync_table()
    rng = np.random.RandomState(8)
    acts_host = rng.choice(6, size=(3, 4, n), p=[.18, .18, .18, .18, .18, .10]).astype(np.int32)
    acts = torch.zeros((4, n), dtype=torch.int32, device="cuda")
    outs = [lang_stream_buffers(a) for _ in range(4)]
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            for k in range(4):
                a.step_lang_stream(acts[k], tick=k, **outs[k])
    restarts = 0
    for r in range(3):
        acts.copy_(torch.as_tensor(acts_host[r]))
        for o in outs:
            o["any_live"].zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in range(4):
            ob = lang_stream_buffers(b)
            b.step_lang_stream(torch.as_tensor(acts_host[r, k], device="cuda"), tick=k, **ob)
            for name in LANG_STREAM_OUTPUTS + ("any_live",):
                assert torch.equal(outs[k][name], ob[name]), (name, r, k)
            restarts += int((ob["episode_end"] >= 0).sum())
    assert restarts > n
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.stats(), b.stats())
    assert int(a.error_word()[0]) == int(b.error_word()[0])


@pytest.fixture(scope="module")
def handles():
    return make_handles(0, HANDLES)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_lang_stream_refused(handles, row):
    check_row(handles[row.handle], row)


def test_language_evaluate_equals_language_rollout_gpu(golden):
    check_evaluate_equals_language_rollout(golden, 0)


def test_language_evaluate_equals_reference_gpu(golden):
    check_evaluate_equals_reference(golden, 0)
