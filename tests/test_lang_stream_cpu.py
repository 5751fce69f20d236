"""craft_step_lang_stream on the CPU variant of the ABI (include/craft.h): the tick against the
entry points it fuses, the end-on-a-grab known-answer test, a bad action, sharding over handles,
a WIDTH != HEIGHT world, its refusals, and language_rollout.evaluate against
do_language_rollout and against the reference's evaluate of the three language trainers
(tests/golden/language_evaluate.npz).  tests/test_gpu_step_lang_stream.py runs the same checks,
and HIP against this library, on the card."""
import os
import re

import numpy as np
import pytest
import torch

from psketch_amd import _native as N
from tests.helpers import RECT_SHAPES, make_tables, rect_world
from tests.lang_stream_cases import (check_end_on_a_grab, check_lang_against_composition, check_turn_away_times_out,
                                     grab_queue, lang_stream_buffers, turned_away_faces_other)
from tests.lang_stream_refusal_cases import HANDLES, ROWS
from tests.language_evaluate_cases import check_evaluate_equals_language_rollout, check_evaluate_equals_reference
from tests.refusal_cases import check_row, check_valid_tick, make_handles
from tests.stream_cases import T_MAX, queue_inputs
from tests.test_cpu_variant import cpu_sim

W12 = "craft_medium_12x12"
CHECKS_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "psketch_amd", "csrc",
                        "craft_checks_lang_stream.h")


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
def test_step_lang_stream_equals_step_lang_set_state_observe_teacher_cpu(wrap):
    n = 200
    pool, specs = queue_inputs(W12, 12, n)
    a, b = cpu_sim(W12, n, pool, max_timesteps=T_MAX), cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    check_lang_against_composition(a, b, specs, wrap)


def test_step_lang_stream_rect_world_cpu():
    """A WIDTH != HEIGHT world (7 x 13, C = 91: no multiple of 4)."""
    W, H, window, prims = RECT_SHAPES["r7x13"]
    world, n = rect_world(W, H, window, prims), 70
    pool, specs = queue_inputs(world, W, n, H=H)
    a, b = cpu_sim(world, n, pool, max_timesteps=T_MAX), cpu_sim(world, n, pool, max_timesteps=T_MAX)
    check_lang_against_composition(a, b, specs, False, check_cov=False)


def test_end_on_a_grab_cpu():
    n = 70
    pool, specs, found = grab_queue(W12, 12, 12, n)
    assert found == 475
    a, ref = cpu_sim(W12, n, pool, max_timesteps=1), cpu_sim(W12, n, pool, max_timesteps=1)
    check_end_on_a_grab(a, ref, pool, specs)


def test_turn_away_then_use_times_out_cpu():
    n = 70
    pool, specs, _ = grab_queue(W12, 12, 12, n)
    cfg = make_tables(W12, 2)[3]
    keep = np.asarray([turned_away_faces_other(pool, cfg, 12, 12, s) for s in specs])
    specs = np.ascontiguousarray(specs[keep][:n])
    check_turn_away_times_out(cpu_sim(W12, n, pool, max_timesteps=2), specs)


def test_bad_action_leaves_slot_and_cursor_cpu():
    n, bad = 40, 7
    pool, specs = queue_inputs(W12, 12, n)
    sim = cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    sim.set_episode_queue(torch.as_tensor(specs))
    sim.begin_episodes()
    sim.step_lang_stream(torch.zeros(n, dtype=torch.int32), tick=0)
    before = {k: v.clone() for k, v in sim.get_state().items()}
    acts = torch.zeros(n, dtype=torch.int32)
    acts[bad] = 6
    out = lang_stream_buffers(sim)
    sim.step_lang_stream(acts, tick=1, **out)
    after = sim.get_state()
    for k in before:
        assert torch.equal(after[k][bad], before[k][bad]), k
    assert (int(out["done"][bad]), int(out["success"][bad]), int(out["action_record"][bad]),
            int(out["ask_record"][bad]), int(out["transition_code"][bad])) == (0, -1, -1, -1, -1)
    assert (int(out["episode_end"][bad]), int(out["end_pose"][bad]), int(out["episode_now"][bad])) == (-1, -1, bad)
    assert int(out["action_record"][bad - 1]) == 0
    assert sim.stats().tolist()[2] == 2 * n - 1
    with pytest.raises(N.CraftError) as e:
        sim.check()
    assert e.value.status == N.EBADACTION and f"{bad}" in str(e.value)
    # the cursor was not touched: STOP now ends entry `bad` and takes entry bad + n
    acts[:] = N.STOP
    out = lang_stream_buffers(sim)
    sim.step_lang_stream(acts, tick=2, **out)
    assert int(out["episode_end"][bad]) == bad and int(out["episode_now"][bad]) == bad + n
    # use_alt picks the bad action too
    alt = torch.full((n,), -1, dtype=torch.int32)
    ask = torch.zeros(n, dtype=torch.uint8)
    ask[3] = 1
    sim.step_lang_stream(torch.zeros(n, dtype=torch.int32), tick=3, alt_actions=alt, use_alt=ask, **out)
    assert int(out["action_record"][3]) == -1 and int(out["ask_record"][3]) == -1
    with pytest.raises(N.CraftError) as e:
        sim.check()
    assert e.value.status == N.EBADACTION


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
def test_lang_stream_sharding_cpu(wrap):
    """Two handles of n/2 with env_id_base 0 and n/2 and stride n, concatenated, equal one handle
    of n, for hashed-draw actions."""
    n, h = 40, 20
    pool, specs = queue_inputs(W12, 12, n)
    whole = cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    parts = [cpu_sim(W12, h, pool, max_timesteps=T_MAX, env_id_base=b) for b in (0, h)]
    for s in [whole] + parts:
        s.set_episode_queue(torch.as_tensor(specs))
        s.begin_episodes(stride=n, wrap=wrap)
    restarts = 0
    for t in range(26):
        ow = lang_stream_buffers(whole)
        whole.step_lang_stream(None, seed=21, tick=t, **ow)
        op = [lang_stream_buffers(s) for s in parts]
        for s, o in zip(parts, op):
            s.step_lang_stream(None, seed=21, tick=t, **o)
        for k in ow:
            if k == "any_live":
                assert int(ow[k][0]) == max(int(o[k][0]) for o in op), t
            else:
                assert torch.equal(ow[k], torch.cat([o[k] for o in op])), (k, t)
        restarts += int((ow["episode_end"] >= 0).sum())
    assert restarts > n
    sw = whole.get_state()
    sp = [s.get_state() for s in parts]
    for k in sw:
        assert torch.equal(sw[k], torch.cat([x[k] for x in sp])), k
    assert torch.equal(whole.stats(), parts[0].stats() + parts[1].stats())


def test_the_two_stream_ticks_share_one_cursor_cpu():
    n = 40
    pool, specs = queue_inputs(W12, 12, n)
    sim = cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    sim.set_episode_queue(torch.as_tensor(specs))
    sim.begin_episodes()
    stop = torch.full((n,), N.STOP, dtype=torch.int32)
    now = torch.empty(n, dtype=torch.int32)
    sim.step_lang_stream(stop, episode_now=now)
    assert now.tolist() == list(range(n, 2 * n))
    sim.step_stream(stop, episode_now=now)
    assert now.tolist() == list(range(2 * n, 3 * n))
    sim.step_lang_stream(stop, episode_now=now)
    assert now.tolist() == [i if i < len(specs) else -1 for i in range(3 * n, 4 * n)]


@pytest.fixture(scope="module")
def handles():
    return make_handles("cpu", HANDLES)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_lang_stream_refused_cpu(handles, row):
    check_row(handles[row.handle], row)


def test_valid_tick_after_every_lang_stream_refusal_cpu(oracle_mod):
    handles = make_handles("cpu", HANDLES)
    for row in ROWS:
        check_row(handles[row.handle], row)
    check_valid_tick(handles["base"], oracle_mod)
    c = handles["begun"]
    now = c.t(c.n)
    c.sim.step_lang_stream(torch.full((c.n,), N.STOP, dtype=torch.int32), episode_now=now)
    assert now.tolist() == list(range(c.n, 2 * c.n))
    c.sim.check()


def test_every_message_of_the_lang_stream_header_has_a_row():
    with open(CHECKS_H) as f:
        src = "\n".join(line for line in f.read().splitlines() if not line.lstrip().startswith(("#", "//")))
    literals = [m.encode().decode("unicode_escape") for m in re.findall(r'"((?:[^"\\]|\\.)*)"', src)]
    assert len(literals) >= 5, "the message literals were not found"
    texts = [r.message for r in ROWS]
    assert not [lit for lit in literals if not any(lit in t for t in texts)]
    whole = [lit for lit in literals if re.match(r"craft_\w+: ", lit)]
    assert len(whole) == 4 and not [lit for lit in whole if lit not in texts]


def test_language_evaluate_equals_language_rollout_cpu(golden):
    check_evaluate_equals_language_rollout(golden, "cpu")


def test_language_evaluate_equals_reference_cpu(golden):
    check_evaluate_equals_reference(golden, "cpu")
