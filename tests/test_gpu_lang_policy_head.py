"""The policy head on the language tick, on the card (the tile kernel's MODE_LANG_HEAD /
MODE_LANG_STREAM_HEAD and craft_policy_ask's kernel): the cases of tests/lang_policy_head_cases.py
on the HIP library, the HIP library against the CPU variant bit for bit, sharding, one captured
graph, the language rollout drivers, and the refusals of tests/lang_policy_head_refusal_cases.py."""
import numpy as np
import pytest
import torch

from psketch_amd import CraftSim
from psketch_amd import _native as N
from tests import lang_policy_head_cases as C
from tests import lang_policy_head_refusal_cases as RC
from tests import language_rollout_cases as LC
from tests.helpers import rect_world
from tests.lang_stream_cases import LANG_OUTPUTS
from tests.policy_head_cases import closed_loop_logits, compare_tick, on, world_inputs
from tests.refusal_cases import check_row, make_handles
from tests.stream_cases import T_MAX, queue_inputs
from tests.test_cpu_variant import cpu_sim
from tests.test_gpu_parity import sim_with_pool

pytestmark = pytest.mark.gpu

W12 = "craft_medium_12x12"
W7 = rect_world(16, 12, 7)
# (world, W, H, n): a partial last tile; a single env; w = 5; w = 7
SHAPES = {"n70": (W12, 12, 12, 70), "n1": (W12, 12, 12, 1), "w5_n40": ("craft_large", 10, 10, 40),
          "w7_n40": (W7, 16, 12, 40)}


def test_exports_and_abi_version_gpu():
    for cpu in (True, False):
        L = N.lib(cpu=cpu)
        for name in RC.ENTRIES:
            assert getattr(L, name) is not None
        assert L.craft_abi_version() == 2


def test_policy_ask_equals_the_rule_and_the_cpu_variant():
    L = C.ask_rows()
    gpu = C.check_ask_rule(CraftSim("craft_medium", n_envs=len(L), device=0, pool_capacity=1), L)
    cpu = np.stack([CraftSim("craft_medium", n_envs=len(L), device="cpu", pool_capacity=1)
                    .policy_ask(torch.as_tensor(L), thr).numpy() for thr in C.THRESHOLDS])
    np.testing.assert_array_equal(gpu, cpu)


def pair(shape, other):
    world, W, H, n = SHAPES[shape]
    pool, specs = world_inputs(world, W, n, H=H)
    a = sim_with_pool(world, n, pool, max_timesteps=T_MAX)
    b = sim_with_pool(world, n, pool, max_timesteps=T_MAX) if other == "hip" else cpu_sim(world, n, pool, max_timesteps=T_MAX)
    return a, b, specs


FUSED_ROWS = [(s, m, t, alt, o) for s in SHAPES for m in C.MODES for t in (True, False) for alt in C.ALTS
              for o in ("hip", "cpu")]


@pytest.mark.parametrize("shape,mode,teach,alt,other", FUSED_ROWS,
                         ids=[f"{s}-{m}-{'teach' if t else 'bare'}-{alt}-vs_{o}" for s, m, t, alt, o in FUSED_ROWS])
def test_step_lang_policy_equals_heads_then_step_lang(shape, mode, teach, alt, other):
    """The fused tick against craft_policy_actions on each head + craft_step_lang, on a HIP twin
    and on the CPU variant (the logits are exact on both devices)."""
    a, b, specs = pair(shape, other)
    C.run_lang_fused_vs_split(a, b, specs, mode, teach, alt)


STREAM_ROWS = [(m, w, t, o) for m in C.MODES for w in (False, True) for t in (True, False) for o in ("hip", "cpu")]


@pytest.mark.parametrize("mode,wrap,teach,other", STREAM_ROWS,
                         ids=[f"{m}-{'wrap' if w else 'one_pass'}-{'teach' if t else 'bare'}-vs_{o}"
                              for m, w, t, o in STREAM_ROWS])
def test_step_lang_policy_stream_equals_heads_then_step_lang_stream(mode, wrap, teach, other):
    n = 40
    pool, specs = queue_inputs(W12, 12, n)
    a = sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX) if other == "hip" else cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    C.run_lang_stream_fused_vs_split(a, b, specs, mode, wrap, teach)


def test_lang_sharding():
    pool, specs = world_inputs(W12, 12, 70)

    def make(n, base):
        sim = CraftSim(W12, n_envs=n, device=0, pool_capacity=len(pool), env_id_base=base, max_timesteps=T_MAX)
        sim.load_pool(pool)
        return sim
    C.check_lang_sharding(make, specs)


def test_step_lang_policy_graph():
    """One step_lang tick with logits (both heads, teacher on) captured with torch.cuda.graph and
    replayed three times equals three eager ticks on a twin handle."""
    n = 70
    pool, specs = world_inputs(W12, 12, n)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    obs_a, obs_b = a.empty_obs(), b.empty_obs()
    for s, o in ((a, obs_a), (b, obs_b)):
        s.reset(*specs, obs=o)
        s.sync_table()
    lm = closed_loop_logits(a, C.stop_weights(a.n_features, 7))
    la = closed_loop_logits(a, C.stop_weights(a.n_features, 13))
    ask = on(a, C.ask_mask(n))
    heads = dict(head="sample", head_seed=C.HEAD_SEED, alt_head="sample", alt_head_seed=C.ALT_SEED, use_alt=ask, tick=0)
    oa = C.lang_buffers(a, True)
    oa["obs"] = obs_a
    Lm = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    La = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            a.step_lang(logits=Lm, alt_logits=La, **heads, **oa)
    # (the capture ran nothing: a is still on its reset state; the tick number is the graph's, 0)
    for r in range(3):
        Lm.copy_(lm(obs_a))
        La.copy_(la(obs_a))
        oa["any_live"].zero_()
        g.replay()
        torch.cuda.synchronize()
        ob = C.lang_buffers(b, True)
        ob["obs"] = obs_b
        b.step_lang(logits=lm(obs_b), alt_logits=la(obs_b), **heads, **ob)
        compare_tick(oa, ob, r, LANG_OUTPUTS)
        assert C.compare_lang_handles(a, b, r)[0] == 0
    assert len(set(oa["action_record"].cpu().tolist())) >= 3


@pytest.mark.parametrize("head", C.MODES)
@pytest.mark.parametrize("mode,is_eval,T", LC.CASES, ids=LC.CASE_IDS)
def test_do_language_rollout_head_reproduces_the_reference(golden, monkeypatch, mode, is_eval, T, head):
    fx = golden("language_rollout.npz")
    C.check_case_with_head(monkeypatch, fx, LC.make_sim(fx, T, 0), mode, is_eval, T, head)


def test_language_evaluate_head_equals_argmax_act(golden):
    C.check_language_evaluate_head(golden, 0)


def test_ask_threshold_driver(golden):
    fx = golden("language_rollout.npz")
    C.check_ask_threshold_driver(fx, LC.make_sim(fx, 12, 0))


@pytest.fixture(scope="module")
def handles():
    return make_handles(0, names=RC.HANDLES)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_lang_policy_head_refuses(handles, row):
    check_row(handles[row.handle], row)


def test_handles_still_step_after_the_refusals(handles):
    for name in RC.HANDLES:
        RC.check_still_steps(handles[name])
