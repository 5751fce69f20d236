"""craft_episode_summary (CraftSim.episode_summary): the per-tick records of a queue pass turned
into per-episode results.  Shared by tests/test_episode_summary_cpu.py (the CPU variant) and
tests/test_gpu_episode_summary.py (the HIP library, and HIP against the CPU variant on identical
records).

The expected values never come from the code under test.  Reference 1 is a copy, below, of what
rollout.evaluate did before this entry point existed: the host loop that cut the records
(reference_cut) and the set_state + teacher(path_len_out=) distance loop (reference_distances),
the latter on a handle of its own, so the handle under test is not disturbed.  Reference 2, for
the distances, is the oracle's closest_resource on the entry's initial grid at the end pose.

The dev-split case runs on craft_medium, the 8x8 world the instances of tests/golden/devtest.npz
were generated for (tests/evaluate_cases.py); the other cases run on craft_medium_12x12 and on
rectangular worlds."""
import numpy as np
import torch

from psketch_amd import CraftSim
from psketch_amd import _native as N
from psketch_amd.dataset import Dataset
from psketch_amd.sim import hash_actions
from tests.evaluate_cases import N_ENVS, T_MAX as DEV_T, dev_instances
from tests.helpers import RECT_SHAPES, make_tables
from tests.stream_cases import T_MAX, draw_actions, queue_inputs

W12 = "craft_medium_12x12"
UNTOUCHED = -77                      # the pre-fill of the outputs a test passes in
RECT_SMALLEST = min(RECT_SHAPES, key=lambda t: RECT_SHAPES[t][0] * RECT_SHAPES[t][1])
RECT_LARGEST = "r15x16"              # the largest world the teachers accept: the most BFS words
OUTPUTS = ("length", "success", "end_pose", "distance", "actions", "flags")


def make_sim(world, n, pool, T, device, **kw):
    sim = CraftSim(world, n_envs=n, device=device, pool_capacity=max(1, len(pool)), max_timesteps=T, **kw)
    sim.load_pool(pool)
    return sim


# ---- reference 1: rollout.evaluate's summary as it was before craft_episode_summary -------------
def pose_xyd(p):
    return p & 0xff, (p >> 8) & 0xff, (p >> 16) & 3


def reference_cut(ended, pose, succ, count, rec=None, T=None):
    """rollout._cut_episodes, copied: host arrays [ticks, n] -> length, success (-2: never
    finished), end_pose [count, 3], actions [count, T] padded with -1."""
    length = np.zeros(count, dtype=np.int32)
    success = np.full(count, -2, dtype=np.int8)
    end_pose = np.zeros((count, 3), dtype=np.int32)
    seqs = None if rec is None else np.full((count, T), -1, dtype=np.int32)
    tt, ii = np.nonzero(ended >= 0)
    start = np.zeros(ended.shape[1], dtype=np.int64)
    for t, i in zip(tt, ii):
        e = ended[t, i]
        if e < count:
            length[e] = t + 1 - start[i]
            success[e] = succ[t, i]
            end_pose[e] = pose_xyd(pose[t, i])
            if rec is not None:
                seqs[e, :length[e]] = rec[start[i]:t + 1, i]
        start[i] = t + 1
    return length, success, end_pose, seqs


def reference_distances(probe, specs, success, end_pose):
    """The distance loop rollout._eval_summary ran, copied, on the handle `probe` (same world,
    pool and max_timesteps as the handle under test): set_state on the end poses, then
    teacher(path_len_out=), n_envs at a time.  Entries that never finished keep UNTOUCHED."""
    n, T = probe.n_envs, probe.config.max_timesteps
    goals = np.asarray([t.goal_name == "get" for t in probe.task_manager.tasks])
    is_get = goals[specs[:, 4]]
    distances = np.where(is_get, 0, -1).astype(np.int32)
    failed = np.nonzero(is_get & (success == 0))[0]
    K = probe.n_kinds
    for lo in range(0, len(failed), n):
        idx = failed[lo:lo + n]
        m = len(idx)
        slots = torch.arange(m, dtype=torch.int32, device=probe.device)
        agent = np.concatenate([end_pose[idx], np.full((m, 1), T, dtype=np.int32)], 1)
        probe.set_state(torch.as_tensor(specs[idx]), torch.as_tensor(agent),
                        torch.zeros((m, K), dtype=torch.int32), slots=slots)
        plen = torch.empty(m, dtype=torch.int32, device=probe.device)
        probe.teacher(slots=slots, path_len_out=plen)
        distances[idx] = plen.cpu().numpy()
    try:
        probe.check()
    except N.CraftError as e:
        if e.status != N.ETEACHER:
            raise
    distances[success == -2] = UNTOUCHED
    return distances, is_get


# ---- reference 2: the oracle -------------------------------------------------------------------
def oracle_distances(oracle_mod, cfg, pool, specs, success, end_pose):
    o = oracle_mod.Oracle(cfg, pool)
    is_get = np.asarray([cfg.task[int(t)].goal == N.GOAL_GET for t in specs[:, 4]])
    want = np.where(is_get, 0, -1).astype(np.int32)
    for e in np.nonzero(is_get & (success == 0))[0]:
        probe = o.env(pool[specs[e, 0]], end_pose[e, 0], end_pose[e, 1], end_pose[e, 2])
        rc, _, ln = o.closest_resource(probe, cfg.task[int(specs[e, 4])].arg_kind)
        want[e] = -2 if rc else ln
    want[success == -2] = UNTOUCHED
    return want


# ---- records -------------------------------------------------------------------------------------
def begin(sim, specs, wrap=False):
    """specs (padded with copies of its first row to one entry per slot, as rollout._begin_pass
    pads a short split) installed as the queue, every slot on its first entry.  Returns the
    queue's length."""
    n = sim.n_envs
    queue = specs if len(specs) >= n else np.concatenate([specs, np.repeat(specs[:1], n - len(specs), 0)])
    sim.set_episode_queue(torch.as_tensor(np.ascontiguousarray(queue)))
    obs = sim.empty_obs()
    sim.begin_episodes(first=0, stride=n, wrap=wrap, obs=obs)
    return len(queue), obs


def hash_policy(sim):
    """tests/evaluate_cases.py's integer policy: a hash of the observation (CPU and GPU agree)."""
    w = torch.as_tensor(np.random.RandomState(2).randint(1, 1000, size=sim.n_features), dtype=torch.int64,
                        device=sim.device)
    return lambda obs, t: ((obs.to(torch.int64) * w).sum(1) % 6).to(torch.int32)


def drawn_policy(sim, seed=3):
    rng = np.random.RandomState(seed)
    return lambda obs, t: torch.as_tensor(draw_actions(rng, sim.n_envs), device=sim.device)


def stop_policy(sim):
    return lambda obs, t: torch.full((sim.n_envs,), N.STOP, dtype=torch.int32, device=sim.device)


def stream_pass(sim, specs, policy, lang=False, ticks=None, wrap=False):
    """One-tick launches (craft_step_stream, or with lang craft_step_lang_stream) over the queue
    of `specs` until every slot has run out, or for `ticks` ticks.  Returns the records, device
    tensors [ticks, n]: rec, ended, pose, succ, now."""
    n, dev, T = sim.n_envs, sim.device, sim.config.max_timesteps
    Q, obs = begin(sim, specs, wrap)
    bound = -(-Q // n) * T if ticks is None else ticks
    i32 = dict(dtype=torch.int32, device=dev)
    r = {"rec": torch.full((bound, n), -1, **i32), "ended": torch.full((bound, n), -1, **i32),
         "pose": torch.full((bound, n), -1, **i32), "now": torch.full((bound, n), -1, **i32),
         "succ": torch.full((bound, n), -1, dtype=torch.int8, device=dev)}
    live = torch.zeros(bound, **i32)             # one flag per tick: a tick only ever stores a 1
    step = sim.step_lang_stream if lang else sim.step_stream
    t = 0
    while t < bound:
        step(policy(obs, t), tick=t, obs=obs, success=r["succ"][t], action_record=r["rec"][t],
             any_live=live[t:t + 1], episode_end=r["ended"][t], end_pose=r["pose"][t], episode_now=r["now"][t])
        t += 1
        if ticks is None and int(live[t - 1].cpu()) == 0:
            break
    assert ticks is not None or int(live[t - 1].cpu()) == 0, "the pass did not end"
    sim.check()
    return {k: v[:t] for k, v in r.items()}


def host(records):
    return {k: v.cpu().numpy() for k, v in records.items()}


def on_device(records, sim):
    """Host records as contiguous tensors on sim's device."""
    return {k: torch.as_tensor(np.ascontiguousarray(v)).to(sim.device) for k, v in records.items()}


def summarise(sim, r, count, **kw):
    """sim.episode_summary over the records r, as host arrays (None for an absent output)."""
    out = sim.episode_summary(r["ended"], r["pose"], r["succ"], action_record=r.get("rec"), count=count, **kw)
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def expected(oracle_mod, probe, pool, specs, r, count, T):
    """What episode_summary must return for the host records r over entries [0, count): both
    references' distances agree, entries without an end keep UNTOUCHED as their distance."""
    specs = specs[:count]
    length, success, end_pose, seqs = reference_cut(r["ended"], r["pose"], r["succ"], count, r.get("rec"), T)
    d1, is_get = reference_distances(probe, specs, success, end_pose)
    d2 = oracle_distances(oracle_mod, probe.config, pool, specs, success, end_pose)
    np.testing.assert_array_equal(d1, d2, err_msg="the two references disagree")
    failed = is_get & (success == 0)
    flags = [int((success[success != -2] < 0).any()), int((d1[failed] < 0).any())]
    return {"length": length, "success": success, "end_pose": end_pose, "distance": d1, "actions": seqs,
            "flags": flags, "is_get": is_get}


def assert_equals(got, want, what=""):
    """The summary's host outputs against expected(): an entry without an end must hold the
    binding's pre-fill (length 0, success -2, pose 0, distance -1, actions -1)."""
    done = want["success"] != -2
    np.testing.assert_array_equal(got["length"], want["length"], err_msg=what + " length")
    np.testing.assert_array_equal(got["success"], want["success"], err_msg=what + " success")
    np.testing.assert_array_equal(np.stack(pose_xyd(got["end_pose"]), 1), want["end_pose"], err_msg=what + " pose")
    np.testing.assert_array_equal(got["distance"], np.where(done, want["distance"], -1), err_msg=what + " distance")
    if want["actions"] is not None:
        np.testing.assert_array_equal(got["actions"], want["actions"], err_msg=what + " actions")
    assert got["flags"].tolist() == want["flags"], what + " flags"


def check_pass(oracle_mod, sim, probe, pool, specs, r, count, what=""):
    """One episode_summary call over the device records r against both references; nothing may
    latch.  Returns (got, want)."""
    got = summarise(sim, r, count)
    sim.check()
    want = expected(oracle_mod, probe, pool, specs, host(r), count, sim.config.max_timesteps)
    assert_equals(got, want, what)
    return got, want


# ---- case 1 and 2: the dev split, table on and off -----------------------------------------------
def dev_setup(golden, device):
    ds, items = dev_instances(golden)
    pool = ds.pool_array()
    specs = np.ascontiguousarray(np.stack([np.asarray(a) for a in Dataset.specs(items)], 1).astype(np.int32))
    return pool, specs, make_sim("craft_medium", N_ENVS, pool, DEV_T, device)


def check_dev_split(golden, oracle_mod, device, lang):
    """Case 1: 32 slots over the 150 dev instances, max_timesteps 12, the integer policy of
    tests/evaluate_cases.py, recorded by craft_step_stream (lang: craft_step_lang_stream); every
    output equals both references, and the pass holds the episodes worth checking.  Case 2: the
    same call with the teacher table off gives identical outputs."""
    pool, specs, sim = dev_setup(golden, device)
    probe = make_sim("craft_medium", N_ENVS, pool, DEV_T, device)
    r = stream_pass(sim, specs, hash_policy(sim), lang=lang)
    got, want = check_pass(oracle_mod, sim, probe, pool, specs, r, len(specs), "dev split")
    L, last = want["length"], want["actions"][np.arange(len(specs)), want["length"] - 1]
    assert (want["success"] != -2).all()
    assert ((L == DEV_T) & (last != N.STOP)).any(), "no timed-out episode"
    assert (last == N.STOP).any(), "no STOP episode"
    assert (want["is_get"] & (want["success"] == 1)).any(), "no successful get"
    assert (want["is_get"] & (want["success"] == 0) & (want["distance"] > 0)).any(), "no failed get away from its target"
    sim.tune_teach(table=2)
    off = summarise(sim, r, len(specs))
    sim.check()
    for k in OUTPUTS:
        np.testing.assert_array_equal(off[k], got[k], err_msg=f"table off: {k}")


# ---- case 3: awkward slot counts and densities ---------------------------------------------------
def check_slot_counts(oracle_mod, device, n, rows=None, policy=drawn_policy, ticks=None, repeat=1):
    """n slots on craft_medium_12x12 (max_timesteps 6) over stream_cases' queue of 3n + 17 entries
    (tiled `repeat` times), or over its first `rows` entries (a short split: the queue is padded
    and count < its length).  The outputs sit inside larger tensors pre-filled with UNTOUCHED:
    nothing past entry count - 1 may be written."""
    pool, specs = queue_inputs(W12, 12, n)
    specs = np.ascontiguousarray(np.tile(specs, (repeat, 1)) if rows is None else specs[:rows])
    count = len(specs)
    sim, probe = make_sim(W12, n, pool, T_MAX, device), make_sim(W12, n, pool, T_MAX, device)
    r = stream_pass(sim, specs, policy(sim), ticks=ticks)
    hr = host(r)
    if rows is not None:
        assert (hr["ended"] >= count).any(), "no padding episode ended"
    i32 = dict(dtype=torch.int32, device=sim.device)
    pad = 9
    big = {"length_out": torch.full((count + pad,), UNTOUCHED, **i32),
           "success_out": torch.full((count + pad,), UNTOUCHED, dtype=torch.int8, device=sim.device),
           "end_pose_out": torch.full((count + pad,), UNTOUCHED, **i32),
           "distance_out": torch.full((count + pad,), UNTOUCHED, **i32),
           "actions_out": torch.full((count + pad, T_MAX), UNTOUCHED, **i32)}
    got = summarise(sim, r, count, **{k: v[:count] for k, v in big.items()})
    sim.check()
    for k, v in big.items():
        assert (v[count:] == UNTOUCHED).all(), f"{k} written past entry {count - 1}"
    want = expected(oracle_mod, probe, pool, specs, hr, count, T_MAX)
    done = want["success"] != -2
    # the entries the records end were all written; the others still hold the pre-fill
    for k in ("length", "success", "distance"):
        np.testing.assert_array_equal(got[k][done], want[k][done], err_msg=k)
        assert (got[k][~done] == UNTOUCHED).all(), k
    np.testing.assert_array_equal(np.stack(pose_xyd(got["end_pose"][done]), 1), want["end_pose"][done])
    np.testing.assert_array_equal(got["actions"][done], want["actions"][done])
    assert (got["actions"][~done] == UNTOUCHED).all() and (got["end_pose"][~done] == UNTOUCHED).all()
    assert got["flags"].tolist() == want["flags"]
    return hr, want


def check_every_slot_stops_every_tick(oracle_mod, device, n=70, ticks=8):
    """The densest records: every slot ends an episode every tick."""
    hr, want = check_slot_counts(oracle_mod, device, n, policy=stop_policy, ticks=ticks, repeat=3)
    assert (hr["ended"] >= 0).all() and (want["length"][:ticks * n] == 1).all()
    assert (want["success"][:ticks * n] != -2).all() and (want["success"][ticks * n:] == -2).all()


def check_no_end(device, n=70, ticks=5):
    """Records that hold no end: the outputs stay as they were, and run counts the ticks."""
    pool, specs = queue_inputs(W12, 12, n)
    sim = make_sim(W12, n, pool, T_MAX, device)
    begin(sim, specs)
    i32 = dict(dtype=torch.int32, device=sim.device)
    r = {"ended": torch.full((ticks, n), -1, **i32), "pose": torch.full((ticks, n), -1, **i32),
         "succ": torch.full((ticks, n), -1, dtype=torch.int8, device=sim.device),
         "rec": torch.full((ticks, n), 2, **i32)}
    count = len(specs)
    outs = {"length_out": torch.full((count,), UNTOUCHED, **i32),
            "success_out": torch.full((count,), UNTOUCHED, dtype=torch.int8, device=sim.device),
            "end_pose_out": torch.full((count,), UNTOUCHED, **i32),
            "distance_out": torch.full((count,), UNTOUCHED, **i32),
            "actions_out": torch.full((count, T_MAX), UNTOUCHED, **i32),
            "flags_out": torch.zeros(2, **i32)}
    run = torch.full((n,), 1, **i32)
    got = summarise(sim, r, count, run=run, episode_now=torch.arange(n, **i32), **outs)
    sim.check()
    for k in ("length", "success", "end_pose", "distance"):
        assert (got[k] == UNTOUCHED).all(), k
    assert got["flags"].tolist() == [0, 0]
    assert (run.cpu().numpy() == 1 + ticks).all()
    # the running episodes' actions so far, at their positions (one tick already ran before row 0)
    acts = got["actions"]
    assert (acts[:n, 1:T_MAX] == 2).all() and (acts[:n, 0] == UNTOUCHED).all() and (acts[n:] == UNTOUCHED).all()


# ---- case 4: chunks with carry ------------------------------------------------------------------
def chunk_records(sim, specs, mode, launches=3, K=5, seed=9):
    """launches x K ticks on the queue, ring K: craft_rollout_stream with hashed actions (mode
    'hashed'; it writes no action record, which is rebuilt here from the hashed draw of the slots
    that were running), or craft_rollout_teach_stream with every slot acting on its label (mode
    'label').  Returns the launches' records, each a dict of device tensors [K, n]."""
    n, dev = sim.n_envs, sim.device
    begin(sim, specs)
    i32 = dict(dtype=torch.int32, device=dev)
    label_in = sim.teacher()[0].clone() if mode == "label" else None
    running = np.ones(n, bool)
    chunks = []
    for l in range(launches):
        r = {k: torch.empty((K, n), **i32) for k in ("ended", "pose", "now", "rec")}
        r["succ"] = torch.empty((K, n), dtype=torch.int8, device=dev)
        if mode == "label":
            labels = torch.empty((K, n), **i32)
            sim.rollout_teach_stream(K, seed=seed, tick0=l * K, label_actions=True, label_in=label_in, labels=labels,
                                     action_record=r["rec"], success=r["succ"], episode_end=r["ended"],
                                     end_pose=r["pose"], episode_now=r["now"])
            label_in = labels[K - 1].clone()
        else:
            sim.rollout_stream(K, seed=seed, tick0=l * K, success=r["succ"], episode_end=r["ended"],
                               end_pose=r["pose"], episode_now=r["now"])
            now = r["now"].cpu().numpy()
            rec = np.empty((K, n), dtype=np.int32)
            for k in range(K):
                rec[k] = np.where(running, hash_actions(seed, np.arange(n), l * K + k), -1)
                running = now[k] >= 0
            r["rec"] = torch.as_tensor(rec).to(dev)
        chunks.append(r)
    try:
        sim.check()
    except N.CraftError as e:                  # (label mode: the teacher may raise on a state)
        assert mode == "label" and e.status == N.ETEACHER
    return chunks


def check_chunks(oracle_mod, device, mode, n=40, T=4, K=5):
    """Summarised per launch with run / episode_now carry into the same outputs, against one call
    over the concatenated records and against reference 1: with max_timesteps 4 and 5-tick
    launches most episodes straddle a launch boundary, and their action rows must be complete."""
    pool, specs = queue_inputs(W12, 12, n)
    count = len(specs)
    sim, probe = make_sim(W12, n, pool, T, device), make_sim(W12, n, pool, T, device)
    chunks = chunk_records(sim, specs, mode, K=K)
    i32 = dict(dtype=torch.int32, device=sim.device)
    run = torch.zeros(n, **i32)
    outs, got = {}, None
    for r in chunks:
        res = sim.episode_summary(r["ended"], r["pose"], r["succ"], action_record=r["rec"], count=count, run=run,
                                  episode_now=r["now"][K - 1], **outs)
        outs = {k + "_out": v for k, v in res.items()}
        got = {k: v.cpu().numpy() for k, v in res.items()}
    sim.check()
    whole = {k: torch.cat([r[k] for r in chunks]) for k in chunks[0]}
    run1 = torch.zeros(n, **i32)
    one = summarise(sim, whole, count, run=run1, episode_now=whole["now"][-1])
    sim.check()
    for k in OUTPUTS:
        np.testing.assert_array_equal(got[k], one[k], err_msg=f"per launch against one call: {k}")
    assert torch.equal(run, run1)
    hw = host(whole)
    want = expected(oracle_mod, probe, pool, specs, hw, count, T)
    done = want["success"] != -2
    for k in ("length", "success", "distance", "actions"):
        np.testing.assert_array_equal(got[k][done], want[k][done], err_msg=k)
    np.testing.assert_array_equal(np.stack(pose_xyd(got["end_pose"][done]), 1), want["end_pose"][done])
    assert got["flags"].tolist() == want["flags"]
    # run: the ticks of the episode each slot is still on; 0 for a slot that has run out
    tt = len(hw["ended"])
    last_end = np.where((hw["ended"] >= 0).any(0), tt - 1 - np.argmax(hw["ended"][::-1] >= 0, 0), -1)
    np.testing.assert_array_equal(run.cpu().numpy(), np.where(hw["now"][-1] >= 0, tt - 1 - last_end, 0))
    # the episodes that ended in another launch than they began in
    t_end, i_end = np.nonzero((hw["ended"] >= 0) & (hw["ended"] < count))
    began = t_end + 1 - want["length"][hw["ended"][t_end, i_end]]
    straddle = (began // K) != (t_end // K)
    assert straddle.sum() * 4 >= len(t_end), f"only {straddle.sum()} of {len(t_end)} episodes straddle a launch"
    assert (want["length"][hw["ended"][t_end, i_end]][straddle] > 1).all()


# ---- case 5: rectangular worlds against the oracle -----------------------------------------------
def check_rect(oracle_mod, device, tag, n=24, count=90):
    from tests.rect_cases import rect_case, make_sim as rect_sim
    case = rect_case(oracle_mod, tag, n=count, max_timesteps=T_MAX)
    specs = np.ascontiguousarray(np.stack(case.specs, 1).astype(np.int32))
    sim, probe = rect_sim(case, device, n=n), rect_sim(case, device, n=n)
    r = stream_pass(sim, specs, drawn_policy(sim, seed=case.W * 16 + case.H))
    got, want = check_pass(oracle_mod, sim, probe, case.pool, specs, r, count, tag)
    assert (want["success"] != -2).all()
    assert (want["is_get"] & (want["success"] == 0) & (want["distance"] > 0)).any(), "no failed get away from its target"
    sim.tune_teach(table=2)
    off = summarise(sim, r, count)
    for k in OUTPUTS:
        np.testing.assert_array_equal(off[k], got[k], err_msg=f"{tag}, table off: {k}")


# ---- case 6: flags and latches -------------------------------------------------------------------
FLAG_ROWS = (0, 1, 3)                # flag_setup's doctored pool rows, cycled over its first n entries


def flag_setup(golden, device, n=9):
    """A 12x12 pool with three doctored rows (tests/test_gpu_rollout.py builds such grids for
    craft_rollout_distances): row 0 holds no wood; row 1 one wood walled in by boundary cells, so
    no target can be reached; row 3 a wood in the corner cell (1, 1) and, later in x-major order,
    the same walled one: the case in which find_closest_resources raises (teachers/base.py:31).
    The queue: n `get wood` entries cycling over the three rows, then n more on the untouched
    row 2.  Returns the handle under test, the references' handle, the pool and the queue."""
    pool = np.array(golden("scenarios_seed123.npz")["w12_grids"][:4], dtype=np.uint8)
    _, cb, tm, _ = make_tables(W12)
    wood = next(t.id for t in tm.tasks if str(t) == "get wood")
    for row in FLAG_ROWS:
        pool[row][pool[row] == cb.index["wood"]] = 0
    for row in FLAG_ROWS[1:]:
        g = pool[row].reshape(12, 12)
        g[5, 5] = cb.index["wood"]
        for x, y in ((4, 5), (6, 5), (5, 4), (5, 6)):
            g[x, y] = cb.index["boundary"]
    g = pool[3].reshape(12, 12)
    g[1, 1], g[1, 2], g[2, 1] = cb.index["wood"], 0, 0
    free = [[c for c in range(144) if pool[r][c] == 0 and 2 <= c // 12 <= 10 and 2 <= c % 12 <= 10
             and abs(c // 12 - 5) + abs(c % 12 - 5) > 1] for r in range(4)]
    rows = [FLAG_ROWS[e % 3] if e < n else 2 for e in range(2 * n)]
    specs = np.asarray([[r, free[r][e] // 12, free[r][e] % 12, e % 4, wood] for e, r in enumerate(rows)],
                       dtype=np.int32)
    sim, probe = make_sim(W12, n, pool, T_MAX, device), make_sim(W12, n, pool, T_MAX, device)
    begin(sim, specs)
    return sim, probe, pool, specs


def flag_records(sim, specs, ended, success=0):
    """One tick in which slot i ends entry ended[i] (-1: none) at that entry's start pose."""
    e = np.asarray(ended)
    s = specs[np.clip(e, 0, len(specs) - 1)]
    pose = np.where(e >= 0, s[:, 1] | (s[:, 2] << 8) | (s[:, 3] << 16), -1).astype(np.int32)
    r = {"ended": e[None].astype(np.int32), "pose": pose[None],
         "succ": np.where(e >= 0, success, -1)[None].astype(np.int8), "rec": np.full((1, len(e)), N.STOP, np.int32)}
    return on_device(r, sim)


def check_flags(golden, oracle_mod, device):
    n = 9
    sim, probe, pool, specs = flag_setup(golden, device, n)
    count = len(specs)
    # no target on the row, or none that can be reached: -1; an unreachable target after a reachable
    # one: -2 (craft_rollout_distances' rule, the references'); all set flags[1], nothing latches
    r = flag_records(sim, specs, np.arange(n))
    got = summarise(sim, r, count)
    sim.check()
    want = expected(oracle_mod, probe, pool, specs, host(r), count, T_MAX)
    assert_equals(got, want, "flags")
    assert want["distance"][:n].tolist() == [-1, -1, -2] * (n // 3) and got["flags"].tolist() == [0, 1]
    assert (got["success"][:n] == 0).all() and (got["success"][n:] == -2).all() and (got["length"][:n] == 1).all()
    # the same with the teacher table off
    sim.tune_teach(table=2)
    off = summarise(sim, flag_records(sim, specs, np.arange(n)), count)
    sim.check()
    for k in OUTPUTS:
        np.testing.assert_array_equal(off[k], got[k], err_msg=k)
    sim.tune_teach(table=0)
    # a success of None on an ended episode: flags[0]; a get that did not fail: distance 0
    got = summarise(sim, flag_records(sim, specs, np.arange(n, 2 * n), success=-1), count)
    sim.check()
    assert got["flags"].tolist() == [1, 0] and (got["success"][n:] == -1).all() and (got["distance"][n:] == 0).all()
    # an episode_end past the queue latches CRAFT_ERANGE with the slot; the entry is skipped, and
    # so is one past count (which latches nothing)
    for bad, latches in ((count, True), (count + 5, True), (-2, True), (count - 1, False)):
        ended = np.full(n, -1)
        ended[3], ended[5] = bad, n
        got = summarise(sim, flag_records(sim, specs, ended), count - 1)
        if latches:
            try:
                sim.check()
            except N.CraftError as e:
                assert e.status == N.ERANGE and "3" in str(e), str(e)
            else:
                raise AssertionError(f"episode_end {bad} latched nothing")
        else:
            sim.check()
        assert (got["success"] != -2).nonzero()[0].tolist() == [n], bad
    # a pose outside the interior latches CRAFT_EINVAL and gives -2
    r = flag_records(sim, specs, np.arange(n, 2 * n))
    r["pose"][0, 2] = 0 | (3 << 8)
    got = summarise(sim, r, count)
    try:
        sim.check()
    except N.CraftError as e:
        assert e.status == N.EINVAL
    else:
        raise AssertionError("a pose on the border latched nothing")
    assert got["distance"][n + 2] == -2 and got["flags"].tolist() == [0, 1]


# ---- rollout.replay's distances ------------------------------------------------------------------
def check_replay_distances(golden, oracle_mod, device, K=5):
    """ReplayInfo.distances (one episode_summary call per 5-tick launch, carried by run) against
    the oracle at the success and end pose replay cut from its own records."""
    from psketch_amd import rollout
    pool, specs, sim = dev_setup(golden, device)
    policy = hash_policy(sim)
    ev = rollout.evaluate(sim, specs, lambda obs, ctx: policy(obs, None))
    info = rollout.replay(sim, specs, [ev.eval_info[e]["actions"] for e in range(len(specs))], ticks_per_launch=K)
    want = oracle_distances(oracle_mod, sim.config, pool, specs, info.success, info.end_pose)
    np.testing.assert_array_equal(info.distances, want)
    assert (want > 0).any() and info.launches > 3


# ---- case 7: the handle is left alone ------------------------------------------------------------
def snapshot(sim):
    return {**{k: v.cpu().numpy() for k, v in sim.get_state().items()}, "stats": sim.stats().cpu().numpy()}


def assert_same_handle(before, after, what):
    assert before.keys() == after.keys()
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=f"{what}: {k} changed")


def check_handle_left_alone(device, n=70, ticks=9):
    """episode_summary in the middle of a pass: every field of get_state and stats() stay equal,
    and the pass goes on as that of a handle that was never summarised."""
    pool, specs = queue_inputs(W12, 12, n)
    a, b = make_sim(W12, n, pool, T_MAX, device), make_sim(W12, n, pool, T_MAX, device)
    ra = stream_pass(a, specs, drawn_policy(a), ticks=ticks)
    stream_pass(b, specs, drawn_policy(b), ticks=ticks)
    assert (ra["now"][-1] >= 0).any() and (ra["ended"] >= 0).any()
    before = snapshot(a)
    summarise(a, ra, len(specs))
    a.check()
    assert_same_handle(before, snapshot(a), "episode_summary")
    assert_same_handle(snapshot(b), snapshot(a), "against a handle never summarised")
    pol_a, pol_b = drawn_policy(a, 5), drawn_policy(b, 5)
    for t in range(ticks, ticks + 3):
        a.step_stream(pol_a(None, t), tick=t)
        b.step_stream(pol_b(None, t), tick=t)
    assert_same_handle(snapshot(b), snapshot(a), "three ticks later")


def check_evaluate_leaves_the_handle(golden, device, lang):
    """rollout.evaluate (lang: language_rollout.evaluate): the state the pass's last tick left
    is the state after evaluate returned.  The state after the last tick is taken at the
    driver's first sim.check(), which follows the tick loop directly (act is called before a
    tick, never after the last one; the wrapped act counts the ticks and shows the snapshot was
    taken after the last of them)."""
    from psketch_amd import language_rollout, rollout
    pool, specs, sim = dev_setup(golden, device)
    policy = hash_policy(sim)
    seen = {"acts": 0}

    def act(obs, ctx):
        assert "state" not in seen, "a tick after the snapshot"
        seen["acts"] += 1
        return policy(obs, None)

    check = sim.check

    def first_check():
        if "state" not in seen:
            seen["state"] = snapshot(sim)
        check()

    sim.check = first_check
    info = (language_rollout if lang else rollout).evaluate(sim, specs, act)
    sim.check = check
    assert seen["acts"] == info.ticks and (info.distances > 0).any()
    assert_same_handle(seen["state"], snapshot(sim), "evaluate")
