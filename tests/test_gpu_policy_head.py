"""The policy head on the card (the tile kernel's MODE_TICK_HEAD / MODE_STREAM_HEAD, tick2_kernel's
head instantiations and craft_policy_actions' kernel): the cases of tests/policy_head_cases.py on the
HIP library, the HIP library against the CPU variant bit for bit, one captured graph, the rollout
drivers, and the refusals of tests/policy_head_refusal_cases.py."""
import numpy as np
import pytest
import torch

from psketch_amd import CraftSim
from psketch_amd import _native as N
from tests import policy_head_cases as C
from tests import policy_head_refusal_cases as RC
from tests.helpers import rect_world
from tests.refusal_cases import check_row, make_handles
from tests.stream_cases import T_MAX, queue_inputs
from tests.test_cpu_variant import cpu_sim
from tests.test_gpu_parity import sim_with_pool

pytestmark = pytest.mark.gpu

W12 = "craft_medium_12x12"
W7 = rect_world(16, 12, 7)


def head_sim(n, base=0, device=0):
    return CraftSim("craft_medium", n_envs=n, device=device, pool_capacity=1, env_id_base=base)


def test_exports_and_abi_version_gpu():
    for cpu in (True, False):
        L = N.lib(cpu=cpu)
        for name in RC.ENTRIES:
            assert getattr(L, name) is not None
        assert L.craft_abi_version() == 2


def test_argmax_equals_torch_and_cpu_variant():
    got = C.check_argmax(head_sim(4096))
    np.testing.assert_array_equal(got, C.check_argmax(head_sim(4096, device="cpu")))


def test_bad_rows_yield_minus_one_and_latch():
    def make(n):
        pool, specs = C.world_inputs(W12, 12, n)
        return sim_with_pool(W12, n, pool, max_timesteps=T_MAX), specs
    C.check_bad_rows(make)


def test_sample_against_the_definition_and_cpu_variant():
    n, base = 20000, 123456789
    L = C.logit_rows(n, seed=4, dominated=True)
    acts = C.sample_actions(head_sim(n, base), L)
    for t in range(3):
        C.check_sample_against_definition(L, acts[t], C.HEAD_SEED, base, t)
    np.testing.assert_array_equal(acts, C.sample_actions(head_sim(n, base, device="cpu"), L))
    # the bad rows too, and an index past 2^31 in the id
    Lb = np.concatenate([C.bad_rows(), L[:56]])
    big = 1 << 33
    g = head_sim(len(Lb), big).policy_actions(torch.as_tensor(Lb, device="cuda"), "sample", seed=C.HEAD_SEED, tick=1).cpu().numpy()
    c = head_sim(len(Lb), big, device="cpu").policy_actions(torch.as_tensor(Lb), "sample", seed=C.HEAD_SEED, tick=1).numpy()
    np.testing.assert_array_equal(g, c)
    assert (g[:len(C.bad_rows())] == -1).all()


def test_sharding():
    C.check_sharding(head_sim)


# (world, W, H, n, teach kernel knob): a partial second tile; the two-tile kernel; a one-lane tile;
# w = 5 (craft_large 10x10); w = 7 (a 16x12 world of tests/helpers.py RECT_SHAPES)
SHAPES = {"n70": (W12, 12, 12, 70, 0), "tick2_n133": (W12, 12, 12, 133, 2), "n1": (W12, 12, 12, 1, 0),
          "w5_n40": ("craft_large", 10, 10, 40, 0), "w7_n40": (W7, 16, 12, 40, 0)}
FUSED_ROWS = [(s, mode, teach, autoreset) for s in SHAPES for mode in C.MODES
              for teach, autoreset in ((True, True), (False, False), (True, False))
              if not (s == "tick2_n133" and not teach)]


def pair(shape, other):
    """The HIP handle of a SHAPES row and its twin: another HIP handle, or the CPU variant."""
    world, W, H, n, kernel = SHAPES[shape]
    pool, specs = C.world_inputs(world, W, n, H=H)
    a = sim_with_pool(world, n, pool, max_timesteps=T_MAX)
    b = sim_with_pool(world, n, pool, max_timesteps=T_MAX) if other == "hip" else cpu_sim(world, n, pool, max_timesteps=T_MAX)
    for s in (a, b):
        if kernel and not s._cpu:
            s.tune_teach(kernel=kernel)
            assert s.step_shape(teach=True) == ("tick2_kernel", 128, 2)
    return a, b, specs


@pytest.mark.parametrize("shape,mode,teach,autoreset", FUSED_ROWS,
                         ids=[f"{s}-{m}-{'teach' if t else 'bare'}-{'autoreset' if a else 'freeze'}" for s, m, t, a in FUSED_ROWS])
def test_step_policy_equals_head_then_step(shape, mode, teach, autoreset):
    a, b, specs = pair(shape, "hip")
    C.run_fused_vs_split(a, b, specs, mode, teach, autoreset)


@pytest.mark.parametrize("shape,mode,teach,autoreset", FUSED_ROWS,
                         ids=[f"{s}-{m}-{'teach' if t else 'bare'}-{'autoreset' if a else 'freeze'}" for s, m, t, a in FUSED_ROWS])
def test_step_policy_hip_equals_cpu_variant(shape, mode, teach, autoreset):
    """The fused HIP tick against the CPU variant's head followed by its tick: every output bit
    for bit (the logits are exact on both devices)."""
    a, b, specs = pair(shape, "cpu")
    C.run_fused_vs_split(a, b, specs, mode, teach, autoreset)


STREAM_ROWS = [(mode, wrap, teach, other) for mode in C.MODES for wrap in (False, True)
               for teach, other in ((True, "hip"), (False, "hip"), (True, "cpu"))]


@pytest.mark.parametrize("mode,wrap,teach,other", STREAM_ROWS,
                         ids=[f"{m}-{'wrap' if w else 'one_pass'}-{'teach' if t else 'bare'}-vs_{o}" for m, w, t, o in STREAM_ROWS])
def test_step_policy_stream_equals_head_then_step_stream(mode, wrap, teach, other):
    n = 40
    pool, specs = queue_inputs(W12, 12, n)
    a = sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX) if other == "hip" else cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    C.run_stream_fused_vs_split(a, b, specs, mode, wrap, teach=teach)


def test_step_policy_graph():
    """One step_policy tick (teacher on) captured with torch.cuda.graph and replayed three times
    equals three eager ticks on a twin handle."""
    n = 70
    pool, specs = C.world_inputs(W12, 12, n)
    a, b = sim_with_pool(W12, n, pool, max_timesteps=T_MAX), sim_with_pool(W12, n, pool, max_timesteps=T_MAX)
    obs_a, obs_b = a.empty_obs(), b.empty_obs()
    for s, o in ((a, obs_a), (b, obs_b)):
        s.reset(*specs, obs=o)
        s.sync_table()
    logits = C.closed_loop_logits(a, C.int_weights(a.n_features))
    oa = C.step_buffers(a, True)
    oa["obs"] = obs_a
    L = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            a.step(logits=L, head="sample", head_seed=C.HEAD_SEED, tick=0, autoreset=True, **oa)
    # (the capture ran nothing: a is still on its reset state; the tick number is the graph's, 0)
    for r in range(3):
        L.copy_(logits(obs_a))
        oa["any_live"].zero_()
        g.replay()
        torch.cuda.synchronize()
        ob = C.step_buffers(b, True)
        ob["obs"] = obs_b
        b.step(logits=logits(obs_b), head="sample", head_seed=C.HEAD_SEED, tick=0, autoreset=True, **ob)
        C.compare_tick(oa, ob, r, C.STEP_OUTPUTS + ("any_live",))
        C.compare_handles(a, b, r)
    assert len(set(oa["action_record"].cpu().tolist())) >= 3


@pytest.mark.parametrize("graph", [0, 4])
@pytest.mark.parametrize("is_eval", [True, False], ids=["eval", "train"])
def test_do_rollout_head_equals_argmax_act(golden, is_eval, graph):
    C.check_do_rollout_head(golden, 0, is_eval, graph=graph)


def test_evaluate_head_equals_argmax_act(golden):
    C.check_evaluate_head(golden, 0)


@pytest.fixture(scope="module")
def handles():
    return make_handles(0, names=RC.HANDLES)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_policy_head_refuses(handles, row):
    check_row(handles[row.handle], row)


def test_handles_still_step_after_the_refusals(handles):
    for name in RC.HANDLES:
        RC.check_still_steps(handles[name])
