"""The policy head on the CPU variant of the ABI (CraftSim(device="cpu")): craft_policy_actions,
craft_step_policy and craft_step_policy_stream (include/craft.h "The head rule") against torch's
argmax, against the rule's definition recomputed in Python integers and float64, against the head
followed by the wrapped entry points, through the rollout drivers, and the refusals of
tests/policy_head_refusal_cases.py.  tests/test_gpu_policy_head.py runs the same cases on the card
and compares the HIP library with this one bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from psketch_amd import CraftSim
from psketch_amd import _native as N
from tests import policy_head_cases as C
from tests import policy_head_refusal_cases as RC
from tests.helpers import rect_world
from tests.refusal_cases import check_row, make_handles
from tests.stream_cases import T_MAX, queue_inputs
from tests.test_cpu_variant import cpu_sim

W12 = "craft_medium_12x12"


def head_sim(n, base=0):
    """A handle for the head alone: craft_policy_actions reads no slot state."""
    return CraftSim("craft_medium", n_envs=n, device="cpu", pool_capacity=1, env_id_base=base)


def test_exports_and_abi_version():
    for cpu in (True, False):
        L = N.lib(cpu=cpu)
        for name in RC.ENTRIES:
            assert name in N.SIGNATURES and getattr(L, name) is not None
        assert L.craft_abi_version() == 2 == N.ABI_VERSION


def test_argmax_equals_torch_cpu():
    C.check_argmax(head_sim(4096))


def test_bad_rows_yield_minus_one_and_latch_cpu():
    def make(n):
        pool, specs = C.world_inputs(W12, 12, n)
        return cpu_sim(W12, n, pool, max_timesteps=T_MAX), specs
    C.check_bad_rows(make)


def test_sample_against_the_definition_cpu():
    n = 20000
    L = C.logit_rows(n, seed=4, dominated=True)
    sim = head_sim(n, base=123456789)
    acts = C.sample_actions(sim, L)
    for t in range(3):
        C.check_sample_against_definition(L, acts[t], C.HEAD_SEED, 123456789, t)
    assert (acts[0] != acts[1]).any() and (acts[1] != acts[2]).any()      # the tick keys the draw
    assert (acts[0] != np.argmax(L, 1)).any()                             # and it is a draw


def test_craft_expf_within_2_pow_minus_21(tmp_path):
    """craft_expf against float64 exp on every 1021st float32 of [-80, 0]: a stand-alone program
    (tests/policy_head_expf.cpp) that includes the CPU variant's translation unit, so it measures
    the function the library runs.  The bound is the issue's: 2^-21 relative, 4 ulp over the
    ~1 ulp a degree-6 polynomial reaches (DESIGN.md records the measured maximum)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "policy_head_expf")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", exe, os.path.join(here, "policy_head_expf.cpp"),
                           os.path.join(here, "..", "psketch_amd", "csrc", "scenario_gen.cpp")])
    out = subprocess.check_output([exe], text=True).split()
    f = dict(zip(out[::2], out[1::2]))
    print(f)
    assert int(f["count"]) == (0xC2A00000 - 0x80000000) // 1021 + 1
    assert float(f["max_rel"]) <= 2.0 ** -21 and float(f["rel_at_minus_80"]) <= 2.0 ** -21
    assert float(f["smallest"]) >= 1.1754944e-38 * 1e3                    # every weight a normal float


def test_sharding_cpu():
    C.check_sharding(head_sim)


FUSED_ROWS = [(mode, teach, autoreset) for mode in C.MODES for teach in (False, True) for autoreset in (False, True)]


@pytest.mark.parametrize("mode,teach,autoreset", FUSED_ROWS,
                         ids=[f"{m}-{'teach' if t else 'bare'}-{'autoreset' if a else 'freeze'}" for m, t, a in FUSED_ROWS])
def test_step_policy_equals_head_then_step_cpu(mode, teach, autoreset):
    n = 70
    pool, specs = C.world_inputs(W12, 12, n)
    a, b = cpu_sim(W12, n, pool, max_timesteps=T_MAX), cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    C.run_fused_vs_split(a, b, specs, mode, teach, autoreset)


@pytest.mark.parametrize("world,W,H,n", [("craft_large", 10, 10, 40), (rect_world(16, 12, 7), 16, 12, 40)],
                         ids=["w5", "w7"])
def test_step_policy_wider_windows_cpu(world, W, H, n):
    pool, specs = C.world_inputs(world, W, n, H=H)
    a, b = cpu_sim(world, n, pool, max_timesteps=T_MAX), cpu_sim(world, n, pool, max_timesteps=T_MAX)
    C.run_fused_vs_split(a, b, specs, "sample", True, True)


@pytest.mark.parametrize("wrap", [False, True], ids=["one_pass", "wrap"])
@pytest.mark.parametrize("mode", C.MODES)
def test_step_policy_stream_equals_head_then_step_stream_cpu(mode, wrap):
    n = 40                                                # 137 entries: slots run out on different ticks
    pool, specs = queue_inputs(W12, 12, n)
    a, b = cpu_sim(W12, n, pool, max_timesteps=T_MAX), cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    C.run_stream_fused_vs_split(a, b, specs, mode, wrap)


@pytest.mark.parametrize("is_eval", [True, False], ids=["eval", "train"])
def test_do_rollout_head_equals_argmax_act_cpu(golden, is_eval):
    C.check_do_rollout_head(golden, "cpu", is_eval)


def test_evaluate_head_equals_argmax_act_cpu(golden):
    C.check_evaluate_head(golden, "cpu")


@pytest.fixture(scope="module")
def handles():
    return make_handles("cpu", names=RC.HANDLES)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_policy_head_refuses_cpu(handles, row):
    check_row(handles[row.handle], row)


def test_handles_still_step_after_the_refusals_cpu(handles):
    for name in RC.HANDLES:
        RC.check_still_steps(handles[name])
