"""Shared by tests/test_lang_policy_head_cpu.py and tests/test_gpu_lang_policy_head.py: the policy
head on the language tick (include/craft.h "The ask rule": craft_policy_ask, craft_step_lang_policy,
craft_step_lang_policy_stream).  The ask rule's rows, its float32 transcription and its float64
definition; the fused tick against craft_policy_actions on each head followed by the wrapped
entry point; sharding; the rollout drivers.  Every function takes the simulators it compares, so
one of them may be the HIP library and the other the CPU variant."""
import functools
import math

import numpy as np
import torch

from psketch_amd import _native as N
from psketch_amd import language_rollout
from psketch_amd.language import PrimitiveLanguageTeacher
from tests import language_rollout_cases as LC
from tests.lang_stream_cases import (LANG_OUTPUTS, LANG_STREAM_OUTPUTS, LangCoverage, ask_mask,
                                     lang_stream_buffers)
from tests.policy_head_cases import (HEAD_SEED, NEG_INF, bad_rows, closed_loop_logits, compare_tick, int_weights,
                                     logit_rows, on)
from tests.stream_cases import T_MAX, host_outputs

MODES = ("argmax", "sample")
ALTS = ("alt_head", "alt_int", "no_alt")
ALT_SEED = HEAD_SEED ^ 0x1234567
THRESHOLDS = (0.0, 0.3, 0.5, 1.0)
ASK_ROWS = 4096
# The issue's margin: craft_expf within 2^-21 relative, six-term sums 6 * 2^-24, so ln S, A / S and
# T each carry under 1e-6 absolute, under 2.5e-6 once divided by ln 6; 1e-5 is four times that.
MARGIN = 1e-5
f32 = np.float32


# ---- the ask rule ----------------------------------------------------------------------------------
def entropy64(L):
    """The float64 definition: the entropy of softmax(row) over ln 6 (NaN for a bad row)."""
    L64 = L.astype(np.float64)
    with np.errstate(all="ignore"):
        m = L64.max(1, keepdims=True)
        w = np.where(np.isneginf(L64), 0.0, np.exp(L64 - m))
        p = w / w.sum(1, keepdims=True)
        h = -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(1) / math.log(6)
    bad = ~(L < np.inf).all(1) | np.isneginf(L).all(1)
    return np.where(bad, np.nan, h)


def ask_rows(n=ASK_ROWS):
    """float32 [n, 6]: logit_rows with dominated rows, of which only a dozen each of the rows whose
    normalised entropy is (nearly) 0 or 1 are kept, since those sit on the thresholds 0 and 1 and
    are excused there; then bad_rows(), the six one-hot rows with -inf elsewhere (H = 0), four
    all-equal rows (H = 1) and rows with one and two masked entries."""
    rng = np.random.RandomState(21)
    special = [bad_rows()]
    one_hot = np.full((6, 6), NEG_INF, dtype=f32)
    one_hot[np.arange(6), np.arange(6)] = [0.0, 1.5, -3.0, 80.0, -90.0, 7.0]
    special.append(one_hot)
    special.append(np.repeat(np.asarray([[0.0], [2.5], [-70.0], [12.0]], dtype=f32), 6, 1))
    masked = (rng.standard_normal((64, 6)) * 2).astype(f32)
    for i in range(64):
        masked[i, rng.choice(6, size=1 + i % 2, replace=False)] = NEG_INF
    special.append(masked)
    special = np.concatenate(special)
    L = logit_rows(2 * n, seed=8, dominated=True)
    h = entropy64(L)
    low, high = np.nonzero(h < 1e-4)[0], np.nonzero(h > 1 - 1e-4)[0]
    drop = np.zeros(len(L), bool)
    drop[low[12:]] = True
    drop[high[12:]] = True
    L = L[~drop][:n - len(special)]
    rows = np.concatenate([special, L])
    assert rows.shape == (n, 6)
    return np.ascontiguousarray(rows[rng.permutation(n)])


def fma32(a, b, c):
    """fmaf on float32 arrays, exactly: the product is exact in float64, the sum is rounded to odd
    there (TwoSum gives its error), and 53 bits >= 2 * 24 + 2 make the final rounding the single one."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.asarray(c, dtype=f32).astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    odd = (s.view(np.int64) & 1) == 1
    fix = (e != 0) & ~odd & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(f32)


def craft_expf32(x):
    """craft_expf of include/craft.h on a float32 array in [-80, 0], operation by operation."""
    x = np.asarray(x, dtype=f32)
    k = np.rint(x * _bits(0x3FB8AA3B))
    r = fma32(k, np.broadcast_to(_bits(0xBF317200), x.shape), x)
    r = fma32(k, np.broadcast_to(_bits(0xB5BFBE8E), x.shape), r)
    p = np.broadcast_to(_bits(0x3AB566C5), x.shape)
    for c in (0x3C0936C6, 0x3D2AAC3F, 0x3E2AAA05, 0x3EFFFFFD, 0x3F800000, 0x3F800000):
        p = fma32(p, r, np.broadcast_to(_bits(c), x.shape))
    return (p.view(np.int32) + (k.astype(np.int32) << 23)).view(f32)


def ask_rule32(L, threshold):
    """The ask rule of include/craft.h transcribed in numpy float32."""
    L = np.asarray(L, dtype=f32)
    n = len(L)
    with np.errstate(all="ignore"):
        bad = ~(L[:, 0] < np.inf)
        m = L[:, 0].copy()
        for k in range(1, 6):
            bad |= ~(L[:, k] < np.inf)
            m = np.where(L[:, k] > m, L[:, k], m)
        dead = bad | (m == -np.inf)
        S = np.zeros(n, dtype=f32)
        A = np.zeros(n, dtype=f32)
        for k in range(6):
            d = (L[:, k] - m).astype(f32)
            dk = np.where(d > f32(-80.0), d, f32(-80.0)).astype(f32)
            masked = (L[:, k] == -np.inf) | dead
            w = np.where(masked, f32(0.0), craft_expf32(np.where(masked, f32(0.0), dk))).astype(f32)
            S = w if k == 0 else (S + w).astype(f32)
            A = np.where(masked, A, fma32(w, np.where(masked, f32(0.0), dk), A)).astype(f32)
        T = f32(threshold) * _bits(0x3FE55860)
        q = (A / np.where(dead, f32(1.0), S)).astype(f32)
        x = (T + q).astype(f32)
        neg = ~(x > 0)
        e_neg = craft_expf32(np.where(neg & ~dead, np.maximum(x, f32(-80.0)), f32(0.0)))
        e_pos = craft_expf32(np.where(~neg & ~dead, -x, f32(0.0)))
        ask = np.where(neg, S > e_neg, (S * e_pos).astype(f32) > f32(1.0))
    return np.where(dead, 0, ask).astype(np.uint8)


def check_ask_inputs(L):
    """The issue's conditions on the inputs: at most 1 % of the rows are excused at any threshold;
    at 0.3 and 0.5 both outcomes hold on at least 10 % of the rows.  Returns the float64 entropies."""
    h = entropy64(L)
    for thr in THRESHOLDS:
        with np.errstate(invalid="ignore"):
            near = np.abs(h - thr) <= MARGIN
        assert near.sum() <= len(L) // 100, (thr, int(near.sum()))
    for thr in (0.3, 0.5):
        with np.errstate(invalid="ignore"):
            yes = (h > thr).mean()
        assert 0.1 <= yes <= 0.9, (thr, yes)
    assert np.isnan(h).sum() == len(bad_rows())
    return h


def check_ask_rule(sim, L=None):
    """policy_ask on `sim` equals the float32 transcription bit for bit; agrees with the float64
    definition and with torch's Categorical entropy on every row further than MARGIN from the
    threshold; bad rows and all -inf rows give 0.  Returns the [4, n] bits."""
    L = ask_rows() if L is None else L
    h = check_ask_inputs(L)
    ok = ~np.isnan(h)
    ht = np.full(len(L), np.nan)
    # (the reference's own expression, in float32; its NaN for a bad row compares false as the rule's 0 does)
    ht[ok] = (torch.distributions.Categorical(logits=torch.as_tensor(L[ok]), validate_args=False).entropy()
              / math.log(6)).numpy()
    out = []
    for thr in THRESHOLDS:
        got = sim.policy_ask(on(sim, L), thr).cpu().numpy()
        assert got.dtype == np.uint8 and set(got.tolist()) <= {0, 1}
        np.testing.assert_array_equal(got, ask_rule32(L, thr), err_msg=f"threshold {thr}")
        with np.errstate(invalid="ignore"):
            far = ~(np.abs(h - thr) <= MARGIN)
            np.testing.assert_array_equal(got[far], (h > thr)[far].astype(np.uint8), err_msg=f"float64, {thr}")
            np.testing.assert_array_equal(got[far], (ht > thr)[far].astype(np.uint8), err_msg=f"torch, {thr}")
        assert (got[np.isnan(h)] == 0).all()
        out.append(got)
    return np.stack(out)


# ---- fused against split, the language tick ----------------------------------------------------------
def latched(sim):
    """check() of a handle: (status, text), (0, "") when nothing latched; the latch is cleared."""
    try:
        sim.check()
    except N.CraftError as e:
        return e.status, str(e)
    return 0, ""


def compare_lang_handles(a, b, t):
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k].cpu(), sb[k].cpu()), (k, t)
    assert torch.equal(a.stats().cpu(), b.stats().cpu()), t
    la, lb = latched(a), latched(b)
    assert la == lb, t
    return lb


def lang_buffers(sim, teach):
    o = lang_stream_buffers(sim, teach)
    return {k: o[k] for k in LANG_OUTPUTS}


def stop_weights(F, seed):
    W = int_weights(F, seed=seed)
    W[:, N.STOP] += f32(1.0) * (np.arange(F) % 5 == 0)       # STOP now and then
    return W


def heads_of(mode, t):
    """(main mode, main seed, alt mode, alt seed) at tick t.  "sample": the two heads have different
    modes and seeds, and swap modes every tick so that each head samples on some ticks."""
    if mode == "argmax":
        return "argmax", HEAD_SEED, "argmax", ALT_SEED
    return ("sample", HEAD_SEED, "argmax", ALT_SEED) if t % 2 == 0 else ("argmax", HEAD_SEED, "sample", ALT_SEED)


def one_hot_logits(actions, dev):
    """float32 [n, 6]: 0 at the action and -inf elsewhere (an action outside 0..5: all -inf, the
    head's -1).  Argmax and sample both give the action: a masked action is never drawn."""
    a = torch.as_tensor(actions, device=dev).long().reshape(-1)
    L = torch.full((len(a), 6), NEG_INF, dtype=torch.float32, device=dev)
    ok = (a >= 0) & (a < 6)
    L[torch.nonzero(ok).reshape(-1), a[ok]] = 0.0
    return L


def run_lang_fused_vs_split(a, b, specs, mode, teach, alt, ticks=T_MAX + 1):
    """Handle a runs craft_step_lang_policy; its twin b craft_policy_actions on each head, then
    craft_step_lang on the two vectors and the same use_alt.  Logits from each handle's own
    observations (exact integers).  Every LANG_OUTPUTS array every tick, get_state(), stats() and
    the latched error; at tick 1 a NaN main row on a slot that takes its alt action (harmless) and
    on one that takes its main action (CRAFT_EBADACTION, the slot left as it was)."""
    n = a.n_envs
    Wm, Wa = stop_weights(a.n_features, 7), stop_weights(a.n_features, 13)
    lm = [closed_loop_logits(s, Wm) for s in (a, b)]
    la = [closed_loop_logits(s, Wa) for s in (a, b)]
    obs_a, obs_b = a.empty_obs(), b.empty_obs()
    a.reset(*specs, obs=obs_a)
    b.reset(*specs, obs=obs_b)
    ask = None if alt == "no_alt" else ask_mask(n)
    takes_alt = np.zeros(n, bool) if ask is None else ask.astype(bool)
    bad_main = bad_hidden = None          # chosen at tick 1 among the slots still running
    done = np.zeros(n, np.uint8)
    rng = np.random.RandomState(2)
    stops = timeouts = mixed = 0
    steps = np.zeros(n, int)
    for t in range(ticks):
        hm, hs, am, asd = heads_of(mode, t)
        oa, ob = lang_buffers(a, teach), lang_buffers(b, teach)
        oa["obs"], ob["obs"] = obs_a, obs_b
        Lm = [f(o) for f, o in zip(lm, (obs_a, obs_b))]
        La = [f(o) for f, o in zip(la, (obs_a, obs_b))]
        assert torch.equal(Lm[0].cpu(), Lm[1].cpu()) and torch.equal(La[0].cpu(), La[1].cpu()), t
        if t == 1:
            run_main, run_alt = np.nonzero(~takes_alt & (done == 0))[0], np.nonzero(takes_alt & (done == 0))[0]
            bad_main = int(run_main[0]) if len(run_main) else None
            bad_hidden = int(run_alt[-1]) if len(run_alt) else None
            assert n < 40 or (bad_main is not None and (bad_hidden is not None or ask is None))
            for L in Lm:
                for slot in (bad_main, bad_hidden):
                    if slot is not None:
                        L[slot, 2] = float("nan")
        before = {k: v.cpu().numpy().copy() for k, v in b.get_state().items()}
        acts = b.policy_actions(Lm[1], hm, seed=hs, tick=t)
        kw_a, kw_b = {}, {}
        if alt == "alt_head":
            alt_acts = b.policy_actions(La[1], am, seed=asd, tick=t)
            kw_a = dict(alt_logits=La[0], alt_head=am, alt_head_seed=asd, use_alt=on(a, ask))
            kw_b = dict(alt_actions=alt_acts, use_alt=on(b, ask))
        elif alt == "alt_int":
            r = rng.randint(0, 6, size=n).astype(np.int32)
            kw_a = dict(alt_actions=on(a, r), use_alt=on(a, ask))
            kw_b = dict(alt_actions=on(b, r), use_alt=on(b, ask))
        a.step_lang(logits=Lm[0], head=hm, head_seed=hs, tick=t, **kw_a, **oa)
        b.step_lang(acts, tick=t, **kw_b, **ob)
        compare_tick(oa, ob, t, LANG_OUTPUTS)
        status, text = compare_lang_handles(a, b, t)
        rec, done = ob["action_record"].cpu().numpy(), ob["done"].cpu().numpy()
        if t == 1 and bad_main is not None:
            # a selected bad row: latched, naming the slot, and the slot as it was
            assert int(acts[bad_main]) == -1
            assert status == N.EBADACTION and f"(slot/item {bad_main})" in text, (status, text)
            after = b.get_state()
            for k in before:
                np.testing.assert_array_equal(after[k][bad_main].cpu().numpy(), before[k][bad_main], err_msg=k)
            assert rec[bad_main] == -1
        else:
            assert status == 0, (t, text)             # (a bad main row under use_alt latches nothing)
        if t == 1 and bad_hidden is not None:
            assert int(acts[bad_hidden]) == -1
        stepped = rec >= 0
        steps += stepped
        if ask is not None:
            arec = ob["ask_record"].cpu().numpy()
            mixed += int((arec == 1).any() and (arec == 0).any())
        ended = stepped & (done == 1)
        stops += int((ended & (rec == N.STOP)).sum())
        timeouts += int((ended & (rec != N.STOP)).sum())
    assert (done == 1).all(), "every slot froze and stayed frozen"
    assert stops + timeouts == n
    if n >= 40:
        assert stops > 0 and timeouts > 0, (stops, timeouts)
        assert ask is None or mixed > 0
    return stops, timeouts


# ---- fused against split, on the queue ---------------------------------------------------------------
def run_lang_stream_fused_vs_split(a, b, specs, mode, wrap, teach, ticks=30):
    """The same with craft_step_lang_policy_stream against craft_policy_actions on each head +
    craft_step_lang_stream.  Every third slot (ask_mask) takes the alt head, whose row is 0 at the
    teacher's label of the slot's state and -inf elsewhere, so those slots follow the demonstration
    and some episodes end with their task satisfied; LangCoverage's conditions are asserted from
    b's outputs."""
    n = a.n_envs
    Wm = stop_weights(a.n_features, 7)
    lm = [closed_loop_logits(s, Wm) for s in (a, b)]
    for s in (a, b):
        s.set_episode_queue(torch.as_tensor(specs))
    obs_a, obs_b = a.empty_obs(), b.empty_obs()
    a.begin_episodes(wrap=wrap, obs=obs_a)
    b.begin_episodes(wrap=wrap, obs=obs_b)
    ask = ask_mask(n)
    lab = [a.teacher()[0], b.teacher()[0]]
    cov = LangCoverage(specs, n, wrap)
    names = LANG_STREAM_OUTPUTS + ("any_live",)
    for t in range(ticks):
        hm, hs, am, asd = heads_of(mode, t)
        oa, ob = lang_stream_buffers(a, teach), lang_stream_buffers(b, teach)
        oa["obs"], ob["obs"] = obs_a, obs_b
        Lm = [f(o) for f, o in zip(lm, (obs_a, obs_b))]
        assert torch.equal(Lm[0].cpu(), Lm[1].cpu()), t
        # no label (-1: frozen, -2: the teacher raised): the main row, so that nothing bad is selected
        La = [torch.where(((x >= 0) & (x < 6))[:, None], one_hot_logits(x, s.device), L)
              for x, s, L in zip(lab, (a, b), Lm)]
        acts = b.policy_actions(Lm[1], hm, seed=hs, tick=t)
        alt_acts = b.policy_actions(La[1], am, seed=asd, tick=t)
        a.step_lang_stream(logits=Lm[0], head=hm, head_seed=hs, alt_logits=La[0], alt_head=am, alt_head_seed=asd,
                           use_alt=on(a, ask), tick=t, **oa)
        b.step_lang_stream(acts, alt_actions=alt_acts, use_alt=on(b, ask), tick=t, **ob)
        compare_tick(oa, ob, t, names)
        assert compare_lang_handles(a, b, t)[0] in (0, N.ETEACHER), t
        cov.tick(None, host_outputs(ob))
        lab = [oa["labels"].clone(), ob["labels"].clone()] if teach else [a.teacher()[0], b.teacher()[0]]
    cov.check()
    return cov


# ---- sharding ----------------------------------------------------------------------------------------
def check_lang_sharding(make, specs, n=70, ticks=4):
    """Two handles of n / 2 envs with env_id_base 0 and n / 2 equal one handle of n under sample mode
    on the language tick: make(n, base) -> a handle with the pool loaded; specs: n reset specs."""
    half = n // 2
    whole, parts = make(n, 0), [make(half, 0), make(half, half)]
    obs_w, obs_p = whole.empty_obs(), [p.empty_obs() for p in parts]
    whole.reset(*specs, obs=obs_w)
    for p, o, lo in zip(parts, obs_p, (0, half)):
        p.reset(*[s[lo:lo + half] for s in specs], obs=o)
    Wm, Wa = stop_weights(whole.n_features, 7), stop_weights(whole.n_features, 13)
    ask = ask_mask(n)
    drawn = set()
    for t in range(ticks):
        ow = lang_buffers(whole, True)
        ow["obs"] = obs_w
        whole.step_lang(logits=closed_loop_logits(whole, Wm)(obs_w), head="sample", head_seed=HEAD_SEED, tick=t,
                        alt_logits=closed_loop_logits(whole, Wa)(obs_w), alt_head="sample", alt_head_seed=ALT_SEED,
                        use_alt=on(whole, ask), **ow)
        outs = []
        for p, o, lo in zip(parts, obs_p, (0, half)):
            op = lang_buffers(p, True)
            op["obs"] = o
            p.step_lang(logits=closed_loop_logits(p, Wm)(o), head="sample", head_seed=HEAD_SEED, tick=t,
                        alt_logits=closed_loop_logits(p, Wa)(o), alt_head="sample", alt_head_seed=ALT_SEED,
                        use_alt=on(p, ask[lo:lo + half]), **op)
            outs.append(op)
        for k in LANG_OUTPUTS:
            if k == "any_live":
                assert int(ow[k]) == max(int(o[k]) for o in outs)
            else:
                assert torch.equal(ow[k].cpu(), torch.cat([o[k].cpu() for o in outs])), (k, t)
        drawn |= set(ow["action_record"].cpu().tolist())
    assert len(drawn - {-1}) >= 4, drawn
    whole.check()


# ---- the drivers -------------------------------------------------------------------------------------
class LogitTableStudent(LC.TableStudent):
    """language_rollout_cases.TableStudent returning logits: a row is 0 at the table's action and
    -inf elsewhere, so argmax and sample both return that action."""

    def act(self, obs, t):
        out = super().act(obs, t)
        if isinstance(out, tuple):
            return one_hot_logits(out[0], obs.device), out[1]
        return one_hot_logits(out, obs.device)

    def instructed_act(self, obs, t, ask=None):
        return one_hot_logits(super().instructed_act(obs, t, ask), obs.device)


def check_case_with_head(monkeypatch, fx, sim, mode, is_eval, T, head):
    """language_rollout_cases.check_case, every assertion of it, with the student returning logits
    and the driver given the head."""
    monkeypatch.setattr(LC, "TableStudent", LogitTableStudent)
    monkeypatch.setattr(LC, "do_language_rollout",
                        functools.partial(language_rollout.do_language_rollout, head=head, head_seed=HEAD_SEED))
    return LC.check_case(fx, sim, mode, is_eval, T)


def check_language_evaluate_head(golden, device):
    """language_rollout.evaluate(head="argmax") equals evaluate with an act that takes the argmax, on
    language_evaluate_cases' inputs."""
    from psketch_amd.dataset import Dataset
    from tests.evaluate_cases import N_ENVS, T_MAX as T_EVAL, dev_instances, runner_for
    ds, items = dev_instances(golden)
    runner = runner_for(ds, device)
    sim = runner.sim(N_ENVS)
    logits = closed_loop_logits(sim, stop_weights(sim.n_features, 3))
    specs, ids = Dataset.specs(items), [it["id"] for it in items]
    a = language_rollout.evaluate(sim, specs, lambda obs, ctx: logits(obs), ids=ids, head="argmax")
    b = language_rollout.evaluate(sim, specs, lambda obs, ctx: logits(obs).argmax(dim=1).to(torch.int32), ids=ids)
    assert a.eval_info == b.eval_info and len(a.eval_info) == len(items)
    assert a.success_rate == b.success_rate and a.avg_distance == b.avg_distance and a.ticks == b.ticks
    n_act = np.asarray([len(v["actions"]) for v in a.eval_info.values()])
    assert (n_act == T_EVAL).any() and (n_act < T_EVAL).any()


class EntropyStudent:
    """An active student whose logits are exact integers over 4 of the observation (so they are
    the same on every device) and whose instructed model follows the instruction.  With `thr` it
    computes the ask bits itself (sim.policy_ask); without, act returns the logits alone and the
    driver computes them."""

    def __init__(self, sim, thr=None):
        self.sim, self.thr = sim, thr
        self.logits = closed_loop_logits(sim, stop_weights(sim.n_features, 5))
        self.asks, self.main = [], []

    def init(self, n):
        self.n = n

    def set_tasks(self, task_ids, is_eval):
        pass

    def set_instructions(self, labels):
        self.labels = labels

    def act(self, obs, t):
        L = self.logits(obs)
        self.main.append(L.cpu().numpy().copy())
        if self.thr is None:
            return L
        return L, self.sim.policy_ask(L, self.thr)

    def instructed_act(self, obs, t, ask):
        self.asks.append(ask.cpu().numpy().copy())
        lab = self.labels
        return torch.where(((lab >= 0) & (lab < 6))[:, None], one_hot_logits(lab, obs.device), self.logits(obs))

    def receive(self, descriptions, ask):
        pass

    def terminate(self, done):
        pass

    def imitate_instructed(self):
        pass


def check_ask_threshold_driver(fx, sim, thr=0.9):
    """Active training with ask_threshold: the driver's ask bits equal policy_ask's of the main
    logits, and the rollout equals the same rollout given those bits by the student."""
    infos, students = [], []
    for own in (False, True):
        st = EntropyStudent(sim, thr if own else None)
        info = language_rollout.do_language_rollout(
            sim, fx["spec"].T.copy(), st, PrimitiveLanguageTeacher(np.random.RandomState(LC.SEED)), False, "active",
            head="sample", head_seed=HEAD_SEED, ask_threshold=None if own else thr)
        sim.check()
        infos.append(info.as_info())
        students.append(st)
    drv, own = students
    assert len(drv.asks) == len(own.asks) == len(drv.main) > 1
    for t, (x, y, L) in enumerate(zip(drv.asks, own.asks, drv.main)):
        np.testing.assert_array_equal(x, y, err_msg=f"tick {t}")
        np.testing.assert_array_equal(x, sim.policy_ask(on(sim, L), thr).cpu().numpy(), err_msg=f"tick {t}")
    asks = np.stack(drv.asks)
    assert 0 < asks.mean() < 1, asks.mean()
    assert infos[0] == infos[1]
    assert infos[0]["num_interactions"] > 0
