"""Diagnostic: where a stream tick's time goes.  Per-phase timing of the one-tile tick without a
teacher, craft_step_ex with CRAFT_STEP_AUTORESET against craft_step_stream (wrap on), from the
kernels' s_memrealtime stamps (-DCRAFT_STAMPS, craft_device.h: never the product library).

    python tools/stream_stamps.py --build          # here: libpsketch_craft_diag.so
    python tools/stream_stamps.py [world ...]      # on the GPU: one JSON line per world and side
    python tools/stream_stamps.py --lang [world ...]   # craft_step_lang against craft_step_lang_stream

Phases per workgroup, in microseconds, median and 90th percentile over the grid and the timed
ticks: A (wave 0: state, inventory, mask, action and the scenario row into LDS), C (the protocol,
the transition, and in a stream tick the restart's queue entry and new row), D_wait (the other
waves reach the barrier), D (scatter), E (observation stores); end_max = the last workgroup's end.
--lang: the language protocol's pair.  craft_step_lang has no auto-reset, so its side is reset
every 8 ticks and the ticks right after a reset are dropped like the warm-up ones (its
ending_per_tick is the mean of `done`, which there counts the slots frozen since the reset too)."""
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DIAG = os.path.join(REPO, "psketch_amd", "lib", "libpsketch_craft_diag.so")
if "--build" in sys.argv:
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import diag_build
    diag_build.build(stamped=("craft_sim", "craft_tile", "craft_tick_stream", "craft_tick_lang",
                              "craft_tick_lang_stream"))
    sys.exit(0)
import torch  # noqa: E402
from psketch_amd import _native  # noqa: E402
_native.LIB_PATH = DIAG
from psketch_amd import CraftSim, sample_scenarios, synthetic_specs  # noqa: E402
lib = _native.lib()
lib.craft_debug_set_stamps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
LANG = "--lang" in sys.argv


def run(world, stream, n=65536, ticks=25):
    sim = CraftSim(world, n_envs=n, device=0, pool_capacity=256)
    g, _, _ = sample_scenarios(sim.params, sim.cookbook, 123, 256)
    sim.load_pool(g)
    queue = np.stack(synthetic_specs(g, sim.width, sim.height, 2 * n + 17, 0, 0,
                                     [t.id for t in sim.task_manager.dataset_tasks()]), 1).astype(np.int32)
    if stream:
        sim.set_episode_queue(torch.as_tensor(queue))
        sim.begin_episodes(wrap=True)
    else:
        sim.reset(*[queue[:n, j] for j in range(5)])
    rows = (n + sim.tile_shape()[0] - 1) // sim.tile_shape()[0]
    st = torch.zeros((rows, 8), dtype=torch.int64, device="cuda")
    lib.craft_debug_set_stamps(sim._h, ctypes.c_void_p(st.data_ptr()))
    obs = sim.empty_obs()
    done = torch.empty(n, dtype=torch.uint8, device="cuda")
    res, restarts = [], []
    for t in range(ticks):
        if LANG and stream:
            sim.step_lang_stream(None, seed=5, tick=t, obs=obs, done=done)
        elif LANG:
            if t % 8 == 0:
                sim.reset(*[queue[:n, j] for j in range(5)])
            sim.step_lang(None, seed=5, tick=t, obs=obs, done=done)
        elif stream:
            sim.step_stream(None, seed=5, tick=t, obs=obs, done=done)
        else:
            sim.step(None, seed=5, tick=t, obs=obs, done=done, autoreset=True)
        torch.cuda.synchronize()
        s = st.cpu().numpy().astype(np.float64) / 100.0          # 100 MHz -> us
        res.append(s[:, :7] - s[:, 0].min())
        restarts.append(float(done.float().mean()))
    keep = [t for t in range(5, ticks) if not (LANG and not stream and t % 8 == 0)]
    r = np.stack([res[t] for t in keep])
    side = ("lang_stream" if stream else "lang") if LANG else ("stream" if stream else "step")
    out = {"world": world, "side": side, "tile": sim.tile_shape()[0],
           "ending_per_tick": round(float(np.mean([restarts[t] for t in keep])), 4)}
    for nm, (i, j) in zip(["A", "C", "D_wait", "D", "E"], [(0, 1), (1, 3), (3, 4), (4, 5), (5, 6)]):
        d = r[:, :, j] - r[:, :, i]
        out[nm + "_med"] = round(float(np.median(d)), 2)
        out[nm + "_p90"] = round(float(np.percentile(d, 90)), 2)
    out["end_med"] = round(float(np.median(r[:, :, 6])), 2)
    out["end_max"] = round(float(np.median(r[:, :, 6].max(axis=1))), 2)
    sim.check()
    return out


for w in [a for a in sys.argv[1:] if not a.startswith("--")] or ["craft_medium_12x12", "craft_medium_12x12_w5"]:
    for stream in (False, True):
        print(json.dumps(run(w, stream)), flush=True)
