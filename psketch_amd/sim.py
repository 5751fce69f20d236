"""Batched CraftWorld simulator on one MI355X: the Python face of the C ABI.

`CraftSim` owns N environment slots in HBM (struct-of-arrays, see
csrc/craft_sim.hip) and exposes the reference's CraftWorld/CraftState surface
batched over torch device tensors:

  reset(...)         CraftScenario.init           craft.py:262-273
  step(actions)      do_rollout tick + features    trainers/imitation.py:59-73, craft.py:296-424
  transition(a)      CraftState.step               craft.py:332-424
  observe()          CraftState.features/satisfies craft.py:285-330
  teacher()          DemonstrationTeacher.__call__ teachers/demonstration.py:9-30

All work runs in HIP kernels on the caller's current torch stream; outputs are
device tensors the trainer consumes in place (no host round trip).
"""
import ctypes
import weakref

import numpy as np
import torch

from . import _native as N
from .cookbook import Cookbook, TaskManager, compile_config, world_params, generator_primitives
from . import gamedef


def _ptr(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def _put(struct, keep, field, t):
    """Points struct.field at tensor t, which `keep` holds alive until the call returns (None:
    the field stays null)."""
    if t is not None:
        keep.append(t)
        setattr(struct, field, t.data_ptr())


def _ring_extent(named_outputs, n):
    """The ring length R the given [R, N, ...] outputs of a multi-tick launch share (None: no
    output given)."""
    ring = None
    for name, t in named_outputs:
        if t is not None:
            if t.dim() < 1 or t.shape[0] < 1:
                raise ValueError(f"{name} must be a ring [R >= 1, {n}, ...]")
            if ring is not None and t.shape[0] != ring:
                raise ValueError(f"{name} ring {t.shape[0]} != ring {ring} of the other outputs")
            ring = t.shape[0]
    return ring


def _stack_specs(specs):
    """The 5-tuple of arrays Dataset.specs returns as one host [count, 5] array; anything else
    as it came."""
    if isinstance(specs, (tuple, list)) and len(specs) == 5 and np.ndim(specs[0]) == 1:
        return np.stack([np.asarray(torch.as_tensor(a).cpu()) for a in specs], 1)
    return specs


class CraftSim:
    """N CraftWorld environments on one GPU.

    world: a gamedef.WORLDS name ("craft_medium_12x12" is the benchmark world),
    a configs/worlds YAML path or a dict.  recipes / hints: YAML paths or None
    for the built-in tables.  env_id_base: global id of slot 0 (rank * N when
    sharded), which keys every per-env random draw.  device: a GPU index (default:
    the current one) runs the HIP library; device="cpu" runs the CPU variant of the
    same ABI (libpsketch_craft_cpu.so) on host tensors, the same results bit for bit.
    """

    def __init__(self, world="craft_medium_12x12", n_envs=4096, device=None, env_id_base=0,
                 pool_capacity=1024, recipes=None, hints=None,
                 max_timesteps=gamedef.MAX_TIMESTEPS):
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type not in ("cuda", "cpu"):
            raise ValueError(f"device {self.device}: a GPU index or 'cpu'")
        self._cpu = self.device.type == "cpu"
        self._L = N.lib(cpu=self._cpu)
        self.params = world_params(world)
        self.cookbook = Cookbook(recipes)
        self.task_manager = TaskManager(hints)
        self.config = compile_config(self.params, self.cookbook, self.task_manager, max_timesteps)
        self.width, self.height = self.params["WIDTH"], self.params["HEIGHT"]
        self.n_kinds = self.cookbook.n_kinds
        self.n_features = self.config.n_features
        self.n_envs = int(n_envs)
        self.env_id_base = int(env_id_base)
        self.pool_capacity = int(pool_capacity)
        self.pool_count = 0
        handle = ctypes.c_void_p()
        N.check(self._L.craft_sim_create(ctypes.byref(self.config), self.device.index or 0, self.n_envs,
                                         self.env_id_base, self.pool_capacity,
                                         ctypes.byref(handle)), what="craft_sim_create", L=self._L)
        self._h = handle
        self.obs_format, self.obs_dtype = "f32", torch.float32
        self._rollout_cache = None
        self._teach_cache = None

    # ---- lifetime ---------------------------------------------------------------
    def close(self):
        self._rollout_cache = None
        self._teach_cache = None
        if getattr(self, "_h", None):
            self._L.craft_sim_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tune(self, tile_envs=0, max_resident_per_cu=0, obs_store=0):
        """Tile-kernel geometry and observation-store cache policy (0 write-back,
        1 nontemporal, 2 write-through); results are identical for every setting."""
        self._check(self._L.craft_sim_tune(self._h, int(tile_envs), int(max_resident_per_cu),
                                           int(obs_store)), "craft_sim_tune")

    def tune_rollout(self, chunk_ticks=0, threads=0):
        """Ticks per dynamically scheduled work unit of rollout() (0 = the whole
        launch, the default; -1 = one continuous pipeline per workgroup across
        its tiles) and threads per tile workgroup (0 = the library's default
        shape); results are identical for every setting."""
        self._check(self._L.craft_sim_tune_rollout(self._h, int(chunk_ticks), int(threads)),
                    "craft_sim_tune_rollout")

    def tune_teach(self, kernel=0, lanes=0, table=0):
        """The teacher's knobs (craft_sim_tune_teach; results are identical for every
        setting): kernel = which kernel step(..., labels=) launches (0 the measured best, 1 the
        one-tile kernel, 2 the two-tile kernel, 3x3 windows); lanes = teacher lanes per query
        (0 default, 1, 2 or 4); table = which teachers read the teacher table (0 auto, 1 always,
        2 never: every query runs the BFS)."""
        self._check(self._L.craft_sim_tune_teach(self._h, int(kernel), int(lanes), int(table)),
                    "craft_sim_tune_teach")

    def tune_host(self, threads=0):
        """Host worker threads of the CPU variant (craft_sim_tune_host: 0 = the machine's);
        validated and ignored by the HIP library. Results are identical for every setting."""
        self._check(self._L.craft_sim_tune_host(self._h, int(threads)), "craft_sim_tune_host")

    def sync_table(self):
        """Build the teacher-table rows of pools loaded since the last teacher launch, on the
        current stream, and wait (craft_sim_sync_table): needed only before capturing a teacher
        launch into a graph right after load_pool (the capture refuses to build them)."""
        self._check(self._L.craft_sim_sync_table(self._h, self._stream()), "craft_sim_sync_table")

    def step_shape(self, teach=False):
        """(kernel name, envs per tile / workgroup, teacher lanes per env) that step()
        launches, without (teach=False) or with labels= (craft_sim_step_shape)."""
        k, e, l = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.craft_sim_step_shape(self._h, int(bool(teach)), ctypes.byref(k),
                                                 ctypes.byref(e), ctypes.byref(l)),
                    "craft_sim_step_shape")
        return N.KERNEL_NAMES[k.value], e.value, l.value

    def rollout_shape(self):
        """(tile_envs, threads, split) the next rollout() launches with, as the
        library resolves its knobs (craft_sim_rollout_shape)."""
        t, nt, sp = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.craft_sim_rollout_shape(self._h, ctypes.byref(t), ctypes.byref(nt),
                                                    ctypes.byref(sp)), "craft_sim_rollout_shape")
        return t.value, nt.value, bool(sp.value)

    def teach_words(self):
        """32-bit words per cell set of the teacher's BFS as the kernels are instantiated (the
        band of columns 1 .. W-2: 8x8 -> 2, 10x10 and 12x12 -> 4, up to 15x15 -> 8)."""
        nw = ((self.width - 2) * self.height + 31) // 32
        return 2 if nw <= 2 else 4 if nw <= 4 else 8

    def tile_shape(self):
        """(tile_envs, obs_store) of the tick kernel (craft_sim_tile_shape)."""
        t, st = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.craft_sim_tile_shape(self._h, ctypes.byref(t), ctypes.byref(st)),
                    "craft_sim_tile_shape")
        return t.value, st.value

    _OBS_FORMATS = {"f32": (N.OBS_F32, torch.float32), "bf16": (N.OBS_BF16, torch.bfloat16),
                    "u8": (N.OBS_U8, torch.uint8)}

    def set_obs_format(self, fmt):
        """Element type of every observation this simulator writes: "f32"
        (default), "bf16" or "u8" — the same exact integer values in each."""
        code, dtype = self._OBS_FORMATS[fmt]
        self._check(self._L.craft_sim_set_obs_format(self._h, code), "craft_sim_set_obs_format")
        self.obs_format, self.obs_dtype = fmt, dtype
        self._rollout_cache = None
        self._teach_cache = None

    def _stream(self):
        # the raw hipStream_t of the caller's current stream on this device (an int; the C ABI's
        # argtypes take it as void*): ~5x cheaper than building a torch.cuda.Stream object.  The
        # CPU variant ignores it.
        if self._cpu:
            return None
        return torch._C._cuda_getCurrentRawStream(self.device.index)

    def _check(self, status, what):
        N.check(status, self._h, what, L=self._L)

    def check(self):
        """Synchronises and raises if a kernel latched an error (bad action,
        teacher assertion, out-of-range slot)."""
        slot = ctypes.c_int64(-1)
        self._check(self._L.craft_sim_check(self._h, ctypes.byref(slot), self._stream()),
                    "kernel error")

    def error_word(self, out=None):
        """Device int32[4] copy of the latched-error record ({status, 0, slot lo, slot hi}),
        queued on the current stream without synchronising (craft_sim_error_word)."""
        if out is None:
            out = torch.empty(4, dtype=torch.int32, device=self.device)
        self._buf("out", out, torch.int32, (4,))
        self._check(self._L.craft_sim_error_word(self._h, _ptr(out), self._stream()),
                    "craft_sim_error_word")
        return out

    # ---- helpers --------------------------------------------------------------------
    def _i32(self, x, n=None):
        if x is None:
            return None
        t = torch.as_tensor(x, device=self.device)
        if t.dtype != torch.int32:
            t = t.to(torch.int32)
        t = t.contiguous()
        if n is not None and t.numel() != n:
            raise ValueError(f"expected {n} entries, got {t.numel()}")
        return t

    def _buf(self, name, t, dtype, shape):
        """Checks a caller-owned output (or input) tensor before its pointer goes
        to the C ABI: dtype, contiguity, exact shape and device.  A wrong buffer
        raises here instead of letting a kernel write out of bounds."""
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
        if t.dtype != dtype:
            raise TypeError(f"{name} is {t.dtype}, expected {dtype}")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the simulator is on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t

    def _put_bufs(self, struct, keep, table):
        """_buf, then _put, for every (field, tensor, dtype, shape) row: the struct's field
        carries the argument's name."""
        for field, t, dtype, shape in table:
            _put(struct, keep, field, self._buf(field, t, dtype, shape))

    def _flag_mask(self, name, x, n):
        """A per-slot flag argument as the uint8 [n] device tensor the ABI takes."""
        m = torch.as_tensor(x, device=self.device)
        m = (m != 0).to(torch.uint8).contiguous() if m.dtype != torch.uint8 else m.contiguous()
        if m.numel() != n:
            raise ValueError(f"{name}: expected {n} entries")
        return m

    def _step_fields(self, st, keep, actions, ref_actions, behavior_clone, obs, reward, done, success,
                     action_record, any_live, transition_code):
        """The pointer fields of a craft_step_args_t (step, step_stream)."""
        n = self.n_envs
        _put(st, keep, "actions", self._i32(actions, n) if actions is not None else None)
        _put(st, keep, "ref_actions", self._i32(ref_actions, n) if ref_actions is not None else None)
        if behavior_clone is not None:
            _put(st, keep, "behavior_clone", self._flag_mask("behavior_clone", behavior_clone, n))
        self._put_bufs(st, keep, (("reward", reward, torch.float32, (n,)),
                                  ("done", done, torch.uint8, (n,)),
                                  ("success", success, torch.int8, (n,)),
                                  ("action_record", action_record, torch.int32, (n,)),
                                  ("any_live", any_live, torch.int32, (1,)),
                                  ("transition_code", transition_code, torch.int8, (n,)),
                                  ("obs", obs, self.obs_dtype, (n, self.n_features))))

    def _lang_fields(self, st, keep, actions, alt_actions, use_alt, obs, done, success, action_record,
                     ask_record, transition_code, any_live, labels):
        """The pointer fields of a craft_lang_step_args_t (step_lang, step_lang_stream)."""
        n = self.n_envs
        if actions is not None:
            _put(st, keep, "actions", self._i32(actions, n))
        if alt_actions is not None:
            _put(st, keep, "alt_actions", self._i32(alt_actions, n))
        if use_alt is not None:
            _put(st, keep, "use_alt", self._flag_mask("use_alt", use_alt, n))
        self._put_bufs(st, keep, (("done", done, torch.uint8, (n,)),
                                  ("success", success, torch.int8, (n,)),
                                  ("action_record", action_record, torch.int32, (n,)),
                                  ("ask_record", ask_record, torch.int8, (n,)),
                                  ("transition_code", transition_code, torch.int8, (n,)),
                                  ("any_live", any_live, torch.int32, (1,)),
                                  ("label_out", labels, torch.int32, (n,)),
                                  ("obs", obs, self.obs_dtype, (n, self.n_features))))

    def _queue_outs(self, st, keep, shape, episode_end, end_pose, episode_now):
        """The three int32 outputs every stream entry adds, of `shape`: (n,) or (ring, n)."""
        self._put_bufs(st, keep, (("episode_end", episode_end, torch.int32, shape),
                                  ("end_pose", end_pose, torch.int32, shape),
                                  ("episode_now", episode_now, torch.int32, shape)))

    def _rollout_fields(self, st, keep, n_ticks, seed, tick0, flags, actions, obs, reward, done, success,
                        more=(), queue=None, more_on=None):
        """The ring outputs, the actions and the five launch words of a struct-taking K-tick
        rollout (rollout_stream, rollout_teach, rollout_teach_stream): obs [R, N, F] and reward,
        done, success [R, N], then `more` ((field, tensor) rows: the entry's further int32 [R, N]
        outputs, fields of `more_on` where that is not the struct itself), then the queue outputs
        (queue: the struct that holds them, episode_end, end_pose, episode_now).  R is that of
        the first ring given."""
        n = self.n_envs
        named = [("obs", obs), ("reward", reward), ("done", done), ("success", success), *more]
        if queue is not None:
            named += (("episode_end", queue[1]), ("end_pose", queue[2]), ("episode_now", queue[3]))
        ring = _ring_extent(named, n) or 1
        shape = (ring, n)
        self._put_bufs(st, keep, [("obs", obs, self.obs_dtype, (ring, n, self.n_features)),
                                  ("reward", reward, torch.float32, shape),
                                  ("done", done, torch.uint8, shape),
                                  ("success", success, torch.int8, shape)])
        self._put_bufs(st if more_on is None else more_on, keep,
                       [(field, t, torch.int32, shape) for field, t in more])
        if queue is not None:
            self._queue_outs(queue[0], keep, shape, *queue[1:])
        if actions is not None:
            _put(st, keep, "actions", self._i32(actions, n * n_ticks))
        st.action_seed = seed & (2**64 - 1)
        st.tick0 = int(tick0)
        st.n_ticks = int(n_ticks)
        st.flags = flags
        st.ring = int(ring)

    def empty_obs(self, n=None):
        n = self.n_envs if n is None else n
        return torch.empty((n, self.n_features), dtype=self.obs_dtype, device=self.device)

    def _obs(self, obs, n=None):
        """An [n, F] observation buffer in the handle's format (n = n_envs)."""
        n = self.n_envs if n is None else n
        return _ptr(self._buf("obs", obs, self.obs_dtype, (n, self.n_features)))

    # ---- scenario pool -----------------------------------------------------------------
    def load_pool(self, grids, first=0):
        """grids: uint8 [P, W, H] or [P, W*H] kind ids (x-major), host or device."""
        g = np.ascontiguousarray(np.asarray(torch.as_tensor(grids).cpu(), dtype=np.uint8))
        g = g.reshape(g.shape[0], self.width * self.height)
        self._check(self._L.craft_pool_load(self._h, g.ctypes.data_as(ctypes.c_void_p), int(first),
                                            int(g.shape[0])), "craft_pool_load")
        self.pool_count = max(self.pool_count, first + g.shape[0])

    def sample_pool(self, count, seed=123, dedup=True):
        """Generates `count` scenarios with the make_data.py generator
        (RandomState(seed) stream) and loads them; returns (grids, init_pos)."""
        grids, init_pos, _ = sample_scenarios(self.params, self.cookbook, seed, count, dedup)
        self.load_pool(grids)
        return grids, init_pos

    def generate_pool(self, count, seed=0, first=0, scenario_id0=None, init_pos=False):
        """make_data.sample_scenario x count on the GPU, straight into pool rows
        [first, first + count) (include/craft.h craft_pool_generate); scenario s
        draws from a stream keyed by its global id (scenario_id0 + s, default
        first + s).  Returns the device int32 [count, 2] initial positions if
        init_pos, else None."""
        prims = np.ascontiguousarray(generator_primitives(self.cookbook), dtype=np.int32)
        ws = np.asarray([self.cookbook.index["workshop%d" % i] for i in range(self.params["N_WORKSHOPS"])],
                        dtype=np.int32)
        out = torch.empty((count, 2), dtype=torch.int32, device=self.device) if init_pos else None
        sid0 = first if scenario_id0 is None else scenario_id0
        self._check(self._L.craft_pool_generate(
            self._h, ctypes.c_uint64(seed & (2**64 - 1)), int(sid0), int(first), int(count),
            self.cookbook.index["boundary"], prims.ctypes.data_as(ctypes.c_void_p), len(prims),
            self.params["N_PRIMITIVES"], ws.ctypes.data_as(ctypes.c_void_p), len(ws), _ptr(out),
            self._stream()), "craft_pool_generate")
        self.pool_count = max(self.pool_count, first + count)
        return out

    # ---- episodes -----------------------------------------------------------------------
    def reset(self, scenario, pos_x, pos_y, dir, task, obs=None):
        n = self.n_envs
        args = [self._i32(a, n) for a in (scenario, pos_x, pos_y, dir, task)]
        self._args_keepalive = args
        self._check(self._L.craft_reset(self._h, *[_ptr(a) for a in args], self._obs(obs), self._stream()),
                    "craft_reset")
        return obs

    def _head(self, keep, logits, head, head_seed):
        """The craft_policy_head_t of a float32 [N, 6] logits tensor; head: "argmax", "sample" or
        a CRAFT_HEAD_* value (the library refuses any other)."""
        self._buf("logits", logits, torch.float32, (self.n_envs, N.N_ACTIONS))
        hd = N.craft_policy_head_t()
        _put(hd, keep, "logits", logits)
        if isinstance(head, str):
            if head not in N.HEAD_MODES:
                raise ValueError(f"head must be 'argmax' or 'sample', got {head!r}")
            head = N.HEAD_MODES[head]
        hd.mode = int(head)
        hd.seed = int(head_seed) & (2**64 - 1)
        return hd

    def policy_actions(self, logits, mode="argmax", seed=0, tick=0, out=None):
        """The policy head alone (craft_policy_actions): int32 [N] actions of float32 [N, 6]
        logits, -1 for a row with a NaN or +inf or nothing but -inf.  mode "argmax": the first
        maximum; "sample": a draw from the softmax keyed by (seed, global env id, tick), the
        same on every device and for every sharding."""
        if out is None:
            out = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        self._buf("out", out, torch.int32, (self.n_envs,))
        keep = []
        hd = self._head(keep, logits, mode, seed)
        self._check(self._L.craft_policy_actions(self._h, ctypes.byref(hd), int(tick), _ptr(out), self._stream()),
                    "craft_policy_actions")
        return out

    def policy_ask(self, logits, threshold, out=None):
        """The ask rule alone (craft_policy_ask): uint8 [N], 1 where the entropy of
        softmax(logits[i]) over ln 6 exceeds threshold (0 <= threshold <= 1), 0 otherwise and for
        a row with a NaN or +inf or nothing but -inf.  The active language student's
        `entropy / log(6) > threshold` (students/active_primitive_language.py:116-119) as one
        launch, bit-identical on every device."""
        if out is None:
            out = torch.empty(self.n_envs, dtype=torch.uint8, device=self.device)
        self._buf("out", out, torch.uint8, (self.n_envs,))
        keep = []
        hd = self._head(keep, logits, N.HEAD_ARGMAX, 0)     # (mode and seed are not read)
        self._check(self._L.craft_policy_ask(self._h, ctypes.byref(hd), ctypes.c_float(float(threshold)), _ptr(out),
                                             self._stream()), "craft_policy_ask")
        return out

    def _lang_heads(self, keep, actions, alt_actions, logits, head, head_seed, alt_logits, alt_head, alt_head_seed):
        """step_lang / step_lang_stream with logits: (the main head, the alt head or None), as
        ctypes arguments of craft_step_lang_policy* (which refuses actions beside logits,
        alt_actions beside alt_logits and alt_logits without use_alt)."""
        if logits is None:
            raise ValueError("alt_logits needs logits (the main head)")
        hd = self._head(keep, logits, head, head_seed)
        if alt_logits is None:
            return ctypes.byref(hd), None
        return ctypes.byref(hd), ctypes.byref(self._head(keep, alt_logits, alt_head, alt_head_seed))

    def step(self, actions=None, seed=0, tick=0, autoreset=True, obs=None, reward=None, done=None,
             success=None, ref_actions=None, behavior_clone=None, action_record=None,
             any_live=None, transition_code=None, labels=None, logits=None, head="argmax", head_seed=0):
        """One rollout tick for every slot (include/craft.h craft_step / craft_step_ex).
        logits (float32 [N, 6]) in place of actions: the tick chooses each slot's action itself
        (craft_step_policy), head = "argmax" (the first maximum) or "sample" (a draw from the
        softmax keyed by head_seed, the global env id and tick).
        actions: int32 device tensor [N] or None for the in-kernel hashed draw;
        ref_actions + behavior_clone (uint8 [N]): cloned actions; action_record
        (int32 [N]) receives the action taken (-1 for done slots); any_live (a
        one-element int32 device tensor) is set to 1 if a slot is still running.
        labels (int32 [N]): the DemonstrationTeacher's action for every slot's NEW
        state, computed in the same launch (craft_step_teach) — what teacher()
        would return right after this step."""
        n = self.n_envs
        flags = N.STEP_AUTORESET if autoreset else 0
        if logits is None and ref_actions is None and behavior_clone is None and action_record is None \
                and any_live is None and transition_code is None and labels is None:
            # plain tick: the short craft_step entry (least host overhead per launch)
            a = self._i32(actions, n) if actions is not None else None
            r = self._buf("reward", reward, torch.float32, (n,))
            d = self._buf("done", done, torch.uint8, (n,))
            sc = self._buf("success", success, torch.int8, (n,))
            self._check(self._L.craft_step(self._h, _ptr(a), ctypes.c_uint64(seed & (2**64 - 1)),
                                           int(tick), flags, self._obs(obs), _ptr(r),
                                           _ptr(d), _ptr(sc), self._stream()), "craft_step")
            return obs
        args = N.craft_step_args_t()
        keep = []
        self._step_fields(args, keep, actions, ref_actions, behavior_clone, obs, reward, done, success,
                          action_record, any_live, transition_code)
        args.action_seed = seed & (2**64 - 1)
        args.tick = int(tick)
        args.flags = flags
        if logits is not None:
            self._buf("labels", labels, torch.int32, (n,))
            hd = self._head(keep, logits, head, head_seed)
            self._check(self._L.craft_step_policy(self._h, ctypes.byref(args), ctypes.byref(hd), _ptr(labels),
                                                  self._stream()), "craft_step_policy")
        elif labels is not None:
            self._buf("labels", labels, torch.int32, (n,))
            self._check(self._L.craft_step_teach(self._h, ctypes.byref(args), _ptr(labels),
                                                 self._stream()), "craft_step_teach")
        else:
            self._check(self._L.craft_step_ex(self._h, ctypes.byref(args), self._stream()),
                        "craft_step")
        return obs

    def step_lang(self, actions=None, seed=0, tick=0, alt_actions=None, use_alt=None, obs=None,
                  done=None, success=None, action_record=None, ask_record=None,
                  transition_code=None, any_live=None, labels=None, flags=0, logits=None, head="argmax",
                  head_seed=0, alt_logits=None, alt_head="argmax", alt_head_seed=0):
        """One tick of the language trainers' rollout for every slot (include/craft.h
        craft_step_lang): every running slot steps first (STOP too), then its timer drops and
        done latches; success is satisfies() of the new state.  actions: int32 [N] or None for
        the hashed draw; use_alt (uint8 [N]) picks alt_actions (int32 [N]) per slot, the active
        trainer's ASK bit.  logits (float32 [N, 6]) in place of actions: the tick chooses each
        slot's action itself (craft_step_lang_policy), head / head_seed as step's; alt_logits
        in place of alt_actions likewise, under alt_head / alt_head_seed (needs use_alt; seed
        two "sample" heads apart).  Outputs, each optional: done uint8, success int8 (-1 running or
        None), action_record int32 and ask_record int8 (-1 for a slot done before the tick),
        transition_code int8, any_live int32 [1], labels int32 [N]: the DemonstrationTeacher on
        every new state in the same launch (-1 for a slot done before the tick)."""
        args = N.craft_lang_step_args_t()
        keep = []
        self._lang_fields(args, keep, actions, alt_actions, use_alt, obs, done, success, action_record,
                          ask_record, transition_code, any_live, labels)
        args.action_seed = seed & (2**64 - 1)
        args.tick = int(tick)
        args.flags = int(flags)
        if logits is not None or alt_logits is not None:
            hd, alt = self._lang_heads(keep, actions, alt_actions, logits, head, head_seed, alt_logits, alt_head,
                                       alt_head_seed)
            self._check(self._L.craft_step_lang_policy(self._h, ctypes.byref(args), hd, alt, self._stream()),
                        "craft_step_lang_policy")
            return obs
        self._check(self._L.craft_step_lang(self._h, ctypes.byref(args), self._stream()),
                    "craft_step_lang")
        return obs

    # ---- the episode queue ------------------------------------------------------------
    def set_episode_queue(self, specs):
        """Install the episode queue (craft_episode_queue): specs is int32 [count, 5] rows of
        (scenario, x0, y0, dir0, task), or the 5-tuple of arrays Dataset.specs returns.  Every
        entry is checked on the device; an invalid one raises (EINVAL, naming the first) and
        the queue installed before stays.  Synchronous."""
        q = torch.as_tensor(_stack_specs(specs))
        if q.dim() != 2 or q.shape[1] != 5:
            raise ValueError(f"specs must be [count, 5], got {tuple(q.shape)}")
        q = q.to(device=self.device, dtype=torch.int32).contiguous()
        self._check(self._L.craft_episode_queue(self._h, _ptr(q), int(q.shape[0])),
                    "craft_episode_queue")
        self.queue_count = int(q.shape[0])

    def begin_episodes(self, first=0, stride=None, wrap=False, obs=None):
        """Put every slot on its first queue entry (craft_episode_begin): the slot with global
        id g = env_id_base + i starts on entry first + g and later takes first + g + k * stride
        (stride: default n_envs; the total envs of all ranks when sharded).  wrap: indices mod
        count, so the stream never runs out; else a slot past the end freezes.  obs as reset."""
        stride = self.n_envs if stride is None else int(stride)
        self._check(self._L.craft_episode_begin(self._h, int(first), stride,
                                                N.QUEUE_WRAP if wrap else 0, self._obs(obs),
                                                self._stream()), "craft_episode_begin")
        return obs

    def step_stream(self, actions=None, seed=0, tick=0, obs=None, reward=None, done=None,
                    success=None, ref_actions=None, behavior_clone=None, action_record=None,
                    any_live=None, transition_code=None, labels=None, episode_end=None,
                    end_pose=None, episode_now=None, logits=None, head="argmax", head_seed=0):
        """step(autoreset=True) whose restart takes the slot's next queue entry
        (craft_step_stream; with logits in place of actions craft_step_policy_stream, as step), with three more int32 [N] outputs: episode_end (the queue index of
        the episode that ended this tick, else -1), end_pose (x | y << 8 | dir << 16 of its
        final state, else -1) and episode_now (the queue index the slot runs after the tick, -1
        once it has run out).  any_live: some slot is still running after the tick."""
        n = self.n_envs
        args = N.craft_stream_step_args_t()
        keep = []
        st = args.step
        self._step_fields(st, keep, actions, ref_actions, behavior_clone, obs, reward, done, success,
                          action_record, any_live, transition_code)
        st.action_seed = seed & (2**64 - 1)
        st.tick = int(tick)
        st.flags = N.STEP_AUTORESET
        self._put_bufs(args, keep, (("label_out", labels, torch.int32, (n,)),))
        self._queue_outs(args, keep, (n,), episode_end, end_pose, episode_now)
        if logits is not None:
            hd = self._head(keep, logits, head, head_seed)
            self._check(self._L.craft_step_policy_stream(self._h, ctypes.byref(args), ctypes.byref(hd),
                                                         self._stream()), "craft_step_policy_stream")
            return obs
        self._check(self._L.craft_step_stream(self._h, ctypes.byref(args), self._stream()),
                    "craft_step_stream")
        return obs

    def step_lang_stream(self, actions=None, seed=0, tick=0, alt_actions=None, use_alt=None, obs=None,
                         done=None, success=None, action_record=None, ask_record=None,
                         transition_code=None, any_live=None, labels=None, episode_end=None,
                         end_pose=None, episode_now=None, flags=0, logits=None, head="argmax", head_seed=0,
                         alt_logits=None, alt_head="argmax", alt_head_seed=0):
        """step_lang on the episode queue (craft_step_lang_stream; with logits
        craft_step_lang_policy_stream, as step_lang): every running slot steps
        first, the ending tick included, success is satisfies() of the state that step left, and
        a slot whose episode ended then restarts on its next queue entry.  step_lang's arguments
        plus step_stream's three int32 [N] outputs: episode_end, end_pose (the pose AFTER the
        ending step) and episode_now.  labels: -1 for a slot frozen before the tick; a slot that
        restarted gets the teacher's answer for its new initial state and task."""
        n = self.n_envs
        args = N.craft_lang_stream_step_args_t()
        keep = []
        st = args.step
        self._lang_fields(st, keep, actions, alt_actions, use_alt, obs, done, success, action_record,
                          ask_record, transition_code, any_live, labels)
        st.action_seed = seed & (2**64 - 1)
        st.tick = int(tick)
        st.flags = int(flags)
        self._queue_outs(args, keep, (n,), episode_end, end_pose, episode_now)
        if logits is not None or alt_logits is not None:
            hd, alt = self._lang_heads(keep, actions, alt_actions, logits, head, head_seed, alt_logits, alt_head,
                                       alt_head_seed)
            self._check(self._L.craft_step_lang_policy_stream(self._h, ctypes.byref(args), hd, alt, self._stream()),
                        "craft_step_lang_policy_stream")
            return obs
        self._check(self._L.craft_step_lang_stream(self._h, ctypes.byref(args), self._stream()),
                    "craft_step_lang_stream")
        return obs

    def rollout(self, n_ticks, seed=0, tick0=0, actions=None, autoreset=True, obs=None,
                reward=None, done=None, success=None):
        """n_ticks craft_step ticks in one launch (include/craft.h craft_rollout),
        identical to calling step(tick=tick0 + k) n_ticks times.  actions: int32
        [n_ticks, N] or None (hashed); obs: [R, N, F] ring in the obs format
        (tick t writes obs[t % R]); reward / done / success: [R, N] rings."""
        n = self.n_envs
        if n_ticks < 0:
            raise ValueError("n_ticks must be >= 0")
        if actions is None:
            # the same output tensors as the last call (a benchmark or trainer loop): their checks
            # still hold, so only the launch arguments change
            c = self._rollout_cache
            if c is not None and all((r is None and t is None) or (r is not None and r() is t)
                                     for r, t in zip(c[0], (obs, reward, done, success))) \
                    and c[1] == self._ring_sig(obs, reward, done, success):
                self._check(self._rollout_fn(self._h, None, seed & 0xFFFFFFFFFFFFFFFF,
                                             int(tick0), int(n_ticks),
                                             N.STEP_AUTORESET if autoreset else 0, *c[2],
                                             self._stream()), "craft_rollout")
                return obs
        ring = _ring_extent((("obs", obs), ("reward", reward), ("done", done), ("success", success)), n)
        if obs is not None:
            self._buf("obs", obs, self.obs_dtype, (ring, n, self.n_features))
        for name, t, dt in (("reward", reward, torch.float32), ("done", done, torch.uint8),
                            ("success", success, torch.int8)):
            self._buf(name, t, dt, (ring, n) if t is not None else ())
        a = None
        if actions is not None:
            a = self._i32(actions, n * n_ticks)
        self._rollout_fn = self._L.craft_rollout
        self._check(self._rollout_fn(self._h, _ptr(a), ctypes.c_uint64(seed & (2**64 - 1)),
                                     int(tick0), int(n_ticks),
                                     N.STEP_AUTORESET if autoreset else 0, _ptr(obs),
                                     int(ring or 1), _ptr(reward), _ptr(done), _ptr(success),
                                     self._stream()), "craft_rollout")
        if a is None:                   # weak references: the cache keeps no output alive
            self._rollout_cache = (
                tuple(None if t is None else weakref.ref(t) for t in (obs, reward, done, success)),
                self._ring_sig(obs, reward, done, success),
                (_ptr(obs), int(ring or 1), _ptr(reward), _ptr(done), _ptr(success)))
        return obs

    def rollout_stream(self, n_ticks, seed=0, tick0=0, actions=None, obs=None, reward=None,
                       done=None, success=None, episode_end=None, end_pose=None, episode_now=None):
        """n_ticks step_stream ticks in one launch (include/craft.h craft_rollout_stream),
        identical to calling step_stream(tick=tick0 + k) n_ticks times: a slot whose episode
        ends restarts on its next queue entry in the middle of the launch.  actions: int32
        [n_ticks, N] or None (hashed); obs: [R, N, F] ring in the obs format (tick t writes
        obs[t % R]); reward / done / success / episode_end / end_pose / episode_now: [R, N]
        rings.  R is that of the first ring given."""
        if n_ticks < 0:
            raise ValueError("n_ticks must be >= 0")
        args = N.craft_rollout_stream_args_t()
        keep = []
        self._rollout_fields(args, keep, n_ticks, seed, tick0, N.STEP_AUTORESET, actions, obs, reward, done,
                             success, queue=(args, episode_end, end_pose, episode_now))
        self._check(self._L.craft_rollout_stream(self._h, ctypes.byref(args), self._stream()),
                    "craft_rollout_stream")
        return obs

    def set_episode_actions(self, actions):
        """Install the recorded action sequences of the installed queue (craft_episode_actions):
        a device or host int tensor [count, max_timesteps], row e = entry e's actions then -1, one
        row per queue entry (the layout of episode_summary's and rollout.demonstrations' action
        arrays).  Every row is checked on the device; an invalid one raises (EINVAL, naming the
        first) and the tape installed before stays.  None drops the tape; set_episode_queue
        drops it too.  Synchronous."""
        if actions is None:
            self._check(self._L.craft_episode_actions(self._h, None, 0), "craft_episode_actions")
            return
        a = torch.as_tensor(actions)
        T = self.config.max_timesteps
        if a.dim() != 2 or a.shape[1] != T:
            raise ValueError(f"actions must be [count, {T}], got {tuple(a.shape)}")
        a = a.to(device=self.device, dtype=torch.int32).contiguous()
        self._check(self._L.craft_episode_actions(self._h, _ptr(a), int(a.shape[0])),
                    "craft_episode_actions")

    def rollout_replay(self, n_ticks, tick0=0, obs=None, reward=None, done=None, success=None,
                       episode_end=None, end_pose=None, episode_now=None, step_now=None,
                       action_next=None):
        """rollout_stream whose actions are the installed tape's (include/craft.h
        craft_rollout_replay): every slot's action is read on the device from its queue entry's
        recorded sequence at the step its timer names, so the launch takes no actions tensor.
        Outputs as rollout_stream's, and two more int32 [R, N] rings of the slot after the tick:
        step_now (actions of its current episode already taken, -1 for a frozen slot) and
        action_next (the action it takes next, -1 for a frozen slot)."""
        if n_ticks < 0:
            raise ValueError("n_ticks must be >= 0")
        args = N.craft_rollout_replay_args_t()
        keep = []
        self._rollout_fields(args.roll, keep, n_ticks, 0, tick0, N.STEP_AUTORESET, None, obs, reward, done,
                             success, more=(("step_now", step_now), ("action_next", action_next)),
                             queue=(args.roll, episode_end, end_pose, episode_now), more_on=args)
        self._check(self._L.craft_rollout_replay(self._h, ctypes.byref(args), self._stream()),
                    "craft_rollout_replay")
        return obs

    def rollout_teach(self, n_ticks, seed=0, tick0=0, actions=None, autoreset=True, obs=None,
                      reward=None, done=None, success=None, labels=None, action_record=None,
                      label_in=None, behavior_clone=None, label_actions=False):
        """n_ticks ticks with the DemonstrationTeacher's label of every slot's new state after
        each one, in one launch (include/craft.h craft_rollout_teach): identical to n_ticks
        step(..., labels=) calls.  Each tick's action per slot: its current state's label when
        label_actions (every slot: make_data's demonstrations) or behavior_clone[i] (uint8 [N]),
        else actions[k] (int32 [n_ticks, N]) or the hashed draw.  label_in (int32 [N]): the
        labels of the states before tick0, needed when labels feed actions (teacher() of the
        reset states, or the previous launch's last labels slot).  Outputs are [R, ...] rings
        (tick t writes slot t % R): obs, reward, done, success, labels (int32), action_record
        (int32, -1 for done slots)."""
        n = self.n_envs
        if n_ticks < 0:
            raise ValueError("n_ticks must be >= 0")
        outs_t = (obs, reward, done, success, labels, action_record)
        if actions is None and label_in is None and behavior_clone is None and not label_actions:
            # the same output rings as the last call (a benchmark loop): their checks still hold
            c = self._teach_cache
            if c is not None and c[1] == self._ring_sig(*outs_t) and all(
                    (r is None and t is None) or (r is not None and r() is t) for r, t in zip(c[0], outs_t)):
                args = c[2]
                args.action_seed = seed & (2**64 - 1)
                args.tick0 = int(tick0)
                args.n_ticks = int(n_ticks)
                args.flags = N.STEP_AUTORESET if autoreset else 0
                self._check(self._L.craft_rollout_teach(self._h, ctypes.byref(args), self._stream()),
                            "craft_rollout_teach")
                return labels
        args = N.craft_rollout_teach_args_t()
        keep = []
        self._rollout_fields(args, keep, n_ticks, seed, tick0, N.STEP_AUTORESET if autoreset else 0, actions,
                             obs, reward, done, success,
                             more=(("labels", labels), ("action_record", action_record)))
        if label_in is not None:
            _put(args, keep, "label_in", self._i32(label_in, n))
        if behavior_clone is not None:
            _put(args, keep, "behavior_clone", self._flag_mask("behavior_clone", behavior_clone, n))
        args.label_actions = 1 if label_actions else 0
        self._check(self._L.craft_rollout_teach(self._h, ctypes.byref(args), self._stream()),
                    "craft_rollout_teach")
        if actions is None and label_in is None and behavior_clone is None and not label_actions:
            # weak references: the cache keeps no output alive
            self._teach_cache = (tuple(None if t is None else weakref.ref(t) for t in outs_t),
                                 self._ring_sig(*outs_t), args)
        return labels

    def rollout_teach_stream(self, n_ticks, seed=0, tick0=0, actions=None, obs=None, reward=None,
                             done=None, success=None, labels=None, action_record=None,
                             label_in=None, behavior_clone=None, label_actions=False,
                             episode_end=None, end_pose=None, episode_now=None):
        """n_ticks step_stream(..., labels=) ticks in one launch (include/craft.h
        craft_rollout_teach_stream): rollout_teach on the episode queue.  A slot whose episode
        ends restarts on its next queue entry in the middle of the launch; its label that tick
        is the teacher's answer for the new initial state and task, which it acts on next tick
        when it acts on labels (label_actions: every slot; behavior_clone[i]: uint8 [N]).
        Otherwise actions[k] (int32 [n_ticks, N]) or the hashed draw.  label_in (int32 [N]): the
        labels of the states before tick0, needed when labels feed actions.  Outputs are [R, ...]
        rings (tick t writes slot t % R): rollout_teach's six and rollout_stream's episode_end,
        end_pose and episode_now (int32)."""
        n = self.n_envs
        if n_ticks < 0:
            raise ValueError("n_ticks must be >= 0")
        args = N.craft_rollout_teach_stream_args_t()
        t = args.teach
        keep = []
        self._rollout_fields(t, keep, n_ticks, seed, tick0, N.STEP_AUTORESET, actions, obs, reward, done,
                             success, more=(("labels", labels), ("action_record", action_record)),
                             queue=(args, episode_end, end_pose, episode_now))
        if label_in is not None:
            _put(t, keep, "label_in", self._i32(label_in, n))
        if behavior_clone is not None:
            _put(t, keep, "behavior_clone", self._flag_mask("behavior_clone", behavior_clone, n))
        t.label_actions = 1 if label_actions else 0
        self._check(self._L.craft_rollout_teach_stream(self._h, ctypes.byref(args), self._stream()),
                    "craft_rollout_teach_stream")
        return labels

    def episode_summary(self, episode_end, end_pose, success, action_record=None, count=None, run=None,
                        episode_now=None, length_out=None, success_out=None, end_pose_out=None,
                        distance_out=None, actions_out=None, flags_out=None, distances=True):
        """The per-episode results of a queue pass (include/craft.h craft_episode_summary): the
        [ticks, N] records the four stream entry points write (episode_end, end_pose int32,
        success int8, action_record int32 or None), rows in tick order, as results indexed by
        queue entry 0 .. count - 1 (default: the whole queue).  No slot state is touched.
        Returns a dict of device tensors: length int32 [count], success int8 [count] (-2: the
        records hold no end of the entry), end_pose int32 [count] (x | y << 8 | dir << 16),
        distance int32 [count] (as craft_rollout_distances': -1 not a get task, 0 not failed,
        else find_closest_resources' length on the initial grid at the final pose, -1 where it
        finds no target it can reach and -2 where it raises; None with distances=False), actions int32 [count, max_timesteps]
        padded with -1 (None without action_record) and flags int32 [2] (a None success; a
        failed get without a reachable target).  Outputs not passed in are allocated, success
        pre-filled with -2 and actions with -1; ones passed in are written where the records
        hold an end and otherwise left as they are; flags is zeroed unless passed in.
        run (int32 [N], in/out) and episode_now (int32 [N], the episode_now row of the records'
        last tick) carry episodes across calls over consecutive launches' records: run holds the
        ticks each slot's current episode has already run, and an episode's action row is
        completed by the call that sees its end."""
        n, dev, T = self.n_envs, self.device, self.config.max_timesteps
        if episode_end is None or episode_end.dim() != 2:
            raise ValueError(f"episode_end must be [ticks, {n}]")
        ticks = int(episode_end.shape[0])
        count = int(getattr(self, "queue_count", 0) if count is None else count)
        rows = (ticks, n)
        args = N.craft_episode_summary_args_t()
        keep = []
        i32 = dict(dtype=torch.int32, device=dev)
        if length_out is None:
            length_out = torch.zeros(max(count, 0), **i32)
        if success_out is None:
            success_out = torch.full((max(count, 0),), -2, dtype=torch.int8, device=dev)
        if end_pose_out is None:
            end_pose_out = torch.zeros(max(count, 0), **i32)
        if distance_out is None and distances:
            distance_out = torch.full((max(count, 0),), -1, **i32)
        if actions_out is None and action_record is not None:
            actions_out = torch.full((max(count, 0), T), -1, **i32)
        if flags_out is None:
            flags_out = torch.zeros(2, **i32)
        self._put_bufs(args, keep, (("episode_end", episode_end, torch.int32, rows),
                                    ("end_pose", end_pose, torch.int32, rows),
                                    ("success", success, torch.int8, rows),
                                    ("action_record", action_record, torch.int32, rows),
                                    ("run", run, torch.int32, (n,)),
                                    ("episode_now", episode_now, torch.int32, (n,)),
                                    ("length_out", length_out, torch.int32, (count,)),
                                    ("success_out", success_out, torch.int8, (count,)),
                                    ("end_pose_out", end_pose_out, torch.int32, (count,)),
                                    ("distance_out", distance_out, torch.int32, (count,)),
                                    ("actions_out", actions_out, torch.int32, (count, T)),
                                    ("flags_out", flags_out, torch.int32, (2,))))
        args.ticks = ticks
        args.count = count
        self._check(self._L.craft_episode_summary(self._h, ctypes.byref(args), self._stream()),
                    "craft_episode_summary")
        return {"length": length_out, "success": success_out, "end_pose": end_pose_out,
                "distance": distance_out, "actions": actions_out, "flags": flags_out}

    @staticmethod
    def _ring_sig(*ts):
        """Storage, shape, strides, dtype and device of each output ring (a tensor resized,
        re-strided or re-pointed in place since the last call no longer matches)."""
        return tuple((t.data_ptr(), tuple(t.shape), t.stride(), t.dtype, t.device)
                     if t is not None else None for t in ts)

    def stats(self, reset=False, out=None):
        """Device int64[3] {successes, episodes ended, env-steps}."""
        if out is None:
            out = torch.zeros(3, dtype=torch.int64, device=self.device)
        self._check(self._L.craft_stats(self._h, _ptr(out), int(bool(reset)), self._stream()),
                    "craft_stats")
        return out

    # ---- reference-granular surface ----------------------------------------------------
    def transition(self, actions, src=None, dst=None, codes=None):
        """CraftState.step per item (craft_transition); codes: int8 [n] device
        tensor receiving the describe() transition code of each item."""
        a = self._i32(actions)
        n = a.numel()
        s, d = self._i32(src, n), self._i32(dst, n)
        self._buf("codes", codes, torch.int8, (n,))
        self._check(self._L.craft_transition(self._h, _ptr(s), _ptr(d), _ptr(a), n, _ptr(codes),
                                             self._stream()), "craft_transition")
        return codes

    def observe(self, slots=None, tasks=None, obs=None, sat=None, n=None):
        s = self._i32(slots)
        n = s.numel() if s is not None else (self.n_envs if n is None else n)
        t = self._i32(tasks, n)
        self._buf("sat", sat, torch.int8, (n,))
        self._check(self._L.craft_observe(self._h, _ptr(s), n, _ptr(t), self._obs(obs, n), _ptr(sat),
                                          self._stream()), "craft_observe")
        return obs, sat

    def teacher(self, slots=None, tasks=None, action_out=None, path_len_out=None, n=None):
        s = self._i32(slots)
        n = s.numel() if s is not None else (self.n_envs if n is None else n)
        t = self._i32(tasks, n)
        if action_out is None:
            action_out = torch.empty(n, dtype=torch.int32, device=self.device)
        self._buf("action_out", action_out, torch.int32, (n,))
        self._buf("path_len_out", path_len_out, torch.int32, (n,))
        self._check(self._L.craft_teacher(self._h, _ptr(s), n, _ptr(t), _ptr(action_out),
                                          _ptr(path_len_out), self._stream()), "craft_teacher")
        return action_out, path_len_out

    def get_state(self, slots=None, n=None, fields=("agent", "inventory", "grid", "spec")):
        """Device copies of the requested fields: agent int32 [n, 4] (x, y, dir,
        timer), inventory int32 [n, K], grid uint8 [n, W*H], spec int32 [n, 5]."""
        s = self._i32(slots)
        n = s.numel() if s is not None else (self.n_envs if n is None else n)
        dev = self.device
        shapes = {"agent": ((n, 4), torch.int32), "inventory": ((n, self.n_kinds), torch.int32),
                  "grid": ((n, self.width * self.height), torch.uint8), "spec": ((n, 5), torch.int32)}
        out = {f: torch.empty(shapes[f][0], dtype=shapes[f][1], device=dev) for f in fields}
        self._check(self._L.craft_get_state(self._h, _ptr(s), n, _ptr(out.get("agent")),
                                            _ptr(out.get("inventory")), _ptr(out.get("grid")),
                                            _ptr(out.get("spec")), self._stream()), "craft_get_state")
        return out

    def set_state(self, spec, agent, inventory=None, slots=None):
        sp = self._i32(spec)
        n = sp.shape[0]
        ag = self._i32(agent)
        iv = self._i32(inventory)
        s = self._i32(slots, n)
        self._check(self._L.craft_set_state(self._h, _ptr(s), n, _ptr(sp), _ptr(ag), _ptr(iv),
                                            self._stream()), "craft_set_state")


# ---- host-side inputs ---------------------------------------------------------------------

def sample_scenarios(params, cookbook, seed, count, dedup=True):
    """make_data.sample_scenario (make_data.py:105-144) x count, native and
    bit-exact against numpy's RandomState(seed).  Returns (grids uint8
    [count, W*H], init_pos int32 [count, 2], mt_state uint32[625])."""
    W, H = params["WIDTH"], params["HEIGHT"]
    prims = np.asarray(generator_primitives(cookbook), dtype=np.int32)
    ws = np.asarray([cookbook.index["workshop%d" % i] for i in range(params["N_WORKSHOPS"])],
                    dtype=np.int32)
    grids = np.zeros((count, W * H), dtype=np.uint8)
    init_pos = np.zeros((count, 2), dtype=np.int32)
    mt = np.zeros(625, dtype=np.uint32)
    st = N.lib().craft_sample_scenarios(
        W, H, cookbook.index["boundary"], prims.ctypes.data_as(ctypes.c_void_p), len(prims),
        params["N_PRIMITIVES"], ws.ctypes.data_as(ctypes.c_void_p), len(ws), seed, count,
        int(bool(dedup)), grids.ctypes.data_as(ctypes.c_void_p),
        init_pos.ctypes.data_as(ctypes.c_void_p), mt.ctypes.data_as(ctypes.c_void_p))
    N.check(st, what="craft_sample_scenarios")
    return grids, init_pos, mt


_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash_actions(seed, gids, tick):
    """The in-kernel action draw of craft_step: splitmix64(seed ^ (gid<<20) ^ tick) >> 32 mod 6."""
    g = np.asarray(gids, dtype=np.uint64)
    key = np.uint64(seed) ^ (g << np.uint64(20)) ^ np.uint64(tick)
    return ((splitmix64(key) >> np.uint64(32)) % np.uint64(6)).astype(np.int32)


def synthetic_specs(grids, width, height, n_envs, env_id_base=0, seed=0, task_ids=None):
    """Per-env initial states for synthetic rollouts, keyed by global env id:
    scenario gid mod P, an interior free cell picked by splitmix64, dir 0
    (init_state's default, craft.py:258), task task_ids[gid mod len].
    Returns int32 arrays (scenario, x, y, dir, task)."""
    grids = np.asarray(grids, dtype=np.uint8).reshape(len(grids), width * height)
    P = len(grids)
    gid = np.arange(env_id_base, env_id_base + n_envs, dtype=np.int64)
    scen = (gid % P).astype(np.int64)
    cells = np.arange(width * height)
    cx, cy = cells // height, cells % height
    interior = (cx > 0) & (cx < width - 1) & (cy > 0) & (cy < height - 1)
    free = (grids == 0) & interior[None, :]
    n_free = free.sum(axis=1)
    if (n_free == 0).any():
        raise ValueError("a scenario has no free interior cell")
    # rank of each free cell within its scenario, x-major
    order = np.cumsum(free, axis=1) - 1
    key = (np.uint64(seed) << np.uint64(32)) ^ gid.astype(np.uint64) ^ np.uint64(0xA5A5A5A5A5A5A5A5)
    k = ((splitmix64(key) >> np.uint64(32)) % n_free[scen].astype(np.uint64)).astype(np.int64)
    # cell index of the k-th free cell of each env's scenario
    pick = np.argmax((order[scen] == k[:, None]) & free[scen], axis=1)
    x = (pick // height).astype(np.int32)
    y = (pick % height).astype(np.int32)
    if task_ids is None:
        task_ids = np.arange(1, dtype=np.int32)
    task_ids = np.asarray(task_ids, dtype=np.int32)
    task = task_ids[gid % len(task_ids)].astype(np.int32)
    return scen.astype(np.int32), x, y, np.zeros(n_envs, dtype=np.int32), task
