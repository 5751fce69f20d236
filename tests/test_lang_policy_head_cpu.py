"""The policy head on the language tick, on the CPU variant of the ABI (CraftSim(device="cpu")):
craft_policy_ask, craft_step_lang_policy and craft_step_lang_policy_stream (include/craft.h "The
ask rule") against the rule's float32 transcription, its float64 definition and torch, against the
heads followed by the wrapped entry points, through the language rollout drivers, and the refusals
of tests/lang_policy_head_refusal_cases.py.  tests/test_gpu_lang_policy_head.py runs the same cases
on the card and compares the HIP library with this one bit for bit."""
import numpy as np
import pytest

from psketch_amd import CraftSim
from psketch_amd import _native as N
from tests import lang_policy_head_cases as C
from tests import lang_policy_head_refusal_cases as RC
from tests import language_rollout_cases as LC
from tests.helpers import rect_world
from tests.policy_head_cases import world_inputs
from tests.refusal_cases import check_row, make_handles
from tests.stream_cases import T_MAX, queue_inputs
from tests.test_cpu_variant import cpu_sim

W12 = "craft_medium_12x12"
W7 = rect_world(16, 12, 7)
# (world, W, H, n): a partial last tile; a single env; w = 5; w = 7
SHAPES = {"n70": (W12, 12, 12, 70), "n1": (W12, 12, 12, 1), "w5_n40": ("craft_large", 10, 10, 40),
          "w7_n40": (W7, 16, 12, 40)}


def test_exports_and_abi_version():
    for cpu in (True, False):
        L = N.lib(cpu=cpu)
        for name in RC.ENTRIES:
            assert name in N.SIGNATURES and getattr(L, name) is not None
        assert L.craft_abi_version() == 2 == N.ABI_VERSION


def test_ask_rows_stay_inside_the_issues_bounds():
    L = C.ask_rows()
    assert L.shape == (C.ASK_ROWS, 6) and L.dtype == np.float32
    h = C.check_ask_inputs(L)
    assert (h[~np.isnan(h)] == 0).sum() >= 6 and (np.abs(h - 1) < 1e-12).sum() >= 4
    assert (np.isneginf(L).sum(1) == 1).any() and (np.isneginf(L).sum(1) == 2).any()


def test_transcription_fma_is_exact():
    """fma32 against exact rational arithmetic on seeded operands, halfway cases of the float64
    sum among them."""
    from fractions import Fraction
    rng = np.random.RandomState(0)
    a = (rng.standard_normal(400) * 3).astype(np.float32)
    b = (rng.standard_normal(400) * 3).astype(np.float32)
    c = np.concatenate([(rng.standard_normal(200) * 1e-7).astype(np.float32),
                        (rng.standard_normal(200) * 9).astype(np.float32)])
    got = C.fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        err = abs(exact - Fraction(float(g)))
        assert err <= abs(exact - Fraction(float(lo))) and err <= abs(exact - Fraction(float(hi)))


def test_policy_ask_cpu():
    sim = CraftSim("craft_medium", n_envs=C.ASK_ROWS, device="cpu", pool_capacity=1)
    bits = C.check_ask_rule(sim)
    assert bits[0].sum() > bits[1].sum() > bits[2].sum() > bits[3].sum()


def pair(shape, T=T_MAX):
    world, W, H, n = SHAPES[shape]
    pool, specs = world_inputs(world, W, n, H=H)
    return cpu_sim(world, n, pool, max_timesteps=T), cpu_sim(world, n, pool, max_timesteps=T), specs


FUSED_ROWS = [(s, m, t, alt) for s in SHAPES for m in C.MODES for t in (True, False) for alt in C.ALTS]
FUSED_IDS = [f"{s}-{m}-{'teach' if t else 'bare'}-{alt}" for s, m, t, alt in FUSED_ROWS]


@pytest.mark.parametrize("shape,mode,teach,alt", FUSED_ROWS, ids=FUSED_IDS)
def test_step_lang_policy_equals_heads_then_step_lang_cpu(shape, mode, teach, alt):
    a, b, specs = pair(shape)
    C.run_lang_fused_vs_split(a, b, specs, mode, teach, alt)


STREAM_ROWS = [(m, w, t) for m in C.MODES for w in (False, True) for t in (True, False)]


@pytest.mark.parametrize("mode,wrap,teach", STREAM_ROWS,
                         ids=[f"{m}-{'wrap' if w else 'one_pass'}-{'teach' if t else 'bare'}" for m, w, t in STREAM_ROWS])
def test_step_lang_policy_stream_equals_heads_then_step_lang_stream_cpu(mode, wrap, teach):
    n = 40
    pool, specs = queue_inputs(W12, 12, n)
    a, b = cpu_sim(W12, n, pool, max_timesteps=T_MAX), cpu_sim(W12, n, pool, max_timesteps=T_MAX)
    C.run_lang_stream_fused_vs_split(a, b, specs, mode, wrap, teach)


def test_lang_sharding_cpu():
    pool, specs = world_inputs(W12, 12, 70)

    def make(n, base):
        sim = CraftSim(W12, n_envs=n, device="cpu", pool_capacity=len(pool), env_id_base=base, max_timesteps=T_MAX)
        sim.load_pool(pool)
        return sim
    C.check_lang_sharding(make, specs)


@pytest.mark.parametrize("head", C.MODES)
@pytest.mark.parametrize("mode,is_eval,T", LC.CASES, ids=LC.CASE_IDS)
def test_do_language_rollout_head_reproduces_the_reference_cpu(golden, monkeypatch, mode, is_eval, T, head):
    fx = golden("language_rollout.npz")
    C.check_case_with_head(monkeypatch, fx, LC.make_sim(fx, T, "cpu"), mode, is_eval, T, head)


def test_language_evaluate_head_equals_argmax_act_cpu(golden):
    C.check_language_evaluate_head(golden, "cpu")


def test_ask_threshold_driver_cpu(golden):
    fx = golden("language_rollout.npz")
    C.check_ask_threshold_driver(fx, LC.make_sim(fx, 12, "cpu"))


def test_head_needs_logits_and_threshold_needs_head(golden):
    fx = golden("language_rollout.npz")
    sim = LC.make_sim(fx, 12, "cpu")
    with pytest.raises(ValueError, match="ask_threshold needs a head"):
        C.language_rollout.do_language_rollout(sim, fx["spec"].T.copy(), None, None, False, "active", ask_threshold=0.5)
    st = LC.TableStudent(fx, "interactive", sim.device)          # returns actions, not logits
    with pytest.raises(ValueError, match="logits"):
        C.language_rollout.do_language_rollout(sim, fx["spec"].T.copy(), st, None, True, "interactive", head="argmax")


@pytest.fixture(scope="module")
def handles():
    return make_handles("cpu", names=RC.HANDLES)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_lang_policy_head_refuses_cpu(handles, row):
    check_row(handles[row.handle], row)


def test_handles_still_step_after_the_refusals_cpu(handles):
    for name in RC.HANDLES:
        RC.check_still_steps(handles[name])
