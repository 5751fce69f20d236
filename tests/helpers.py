"""Shared test helpers: compiled configs for the worlds the fixtures use."""
import numpy as np

from psketch_amd import gamedef
from psketch_amd.cookbook import Cookbook, TaskManager, compile_config, world_params


def make_tables(world="craft_medium", max_timesteps=gamedef.MAX_TIMESTEPS, recipes=None, hints=None):
    params = world_params(world)
    cb = Cookbook(recipes)
    tm = TaskManager(hints)
    cfg = compile_config(params, cb, tm, max_timesteps)
    return params, cb, tm, cfg


def world_for(W, window):
    name = {(8, 3): "craft_medium", (12, 3): "craft_medium_12x12",
            (12, 5): "craft_medium_12x12_w5", (10, 5): "craft_large"}[(W, window)]
    return name


def rect_world(W, H, window, prims=2):
    """Params of a world whose WIDTH and HEIGHT differ (gamedef.WORLDS holds squares only);
    CraftSim and make_tables take the dict where they take a world's name."""
    return dict(WIDTH=W, HEIGHT=H, WINDOW_WIDTH=window, WINDOW_HEIGHT=window, N_WORKSHOPS=3,
                N_PRIMITIVES=prims, N_WORLDS=100)


# tag -> (W, H, window, prims): the rectangles the suite runs (tests/test_rect_worlds.py,
# tests/test_gpu_rect_worlds.py).  The teacher's band is (W-2)*H bits in NW = ceil(band/32) words.
RECT_SHAPES = {
    "r7x13": (7, 13, 3, 2),     # C = 91 (not a multiple of 4), nw 3
    "r13x7": (13, 7, 5, 2),     # its transpose, wider window
    "r6x16": (6, 16, 3, 2),     # band = 64 bits: NW 2 exactly full
    "r16x6": (16, 6, 3, 2),     # transpose
    "r10x16": (10, 16, 5, 2),   # band = 128: NW 4 exactly full
    "r12x16": (12, 16, 5, 2),   # band = 160: NW 5 exactly full
    "r16x12": (16, 12, 7, 2),   # nw 6, run as NW 8
    "r15x16": (15, 16, 7, 2),   # largest world the teacher accepts (4WH = 960), nw 7
    "r16x15": (16, 15, 3, 2),   # the same, transposed, on the 3x3 kernels
    "r5x16": (5, 16, 7, 1),     # window wider than the world
    "r16x5": (16, 5, 7, 1),     # window taller than the world
}
RECT_FIXTURE_TAGS = ("r7x13", "r13x7", "r5x16", "r15x16")   # in tests/golden/rect_worlds.npz


def rect_tables(tag, max_timesteps=gamedef.MAX_TIMESTEPS):
    W, H, window, prims = RECT_SHAPES[tag]
    return make_tables(rect_world(W, H, window, prims), max_timesteps)


def row_ids(rows, n_base, added):
    """ids= of parametrize rows (their first value the world) whose last len(added) values are
    knobs added after the first n_base: pytest's own id of the first n_base values, then
    "-<name><value>" for every knob a row sets (non-zero), so a row that sets none keeps the id it
    had before the knobs existed."""
    def one(i, v):
        return v if isinstance(v, str) else str(v) if isinstance(v, (bool, int, float)) else f"world{i}"
    return ["-".join(one(i, v) for v in row[:n_base]) +
            "".join(f"-{name}{v}" for name, v in zip(added, row[n_base:]) if v)
            for i, row in enumerate(rows)]


def pad_inv(inv, K=32):
    inv = np.asarray(inv)
    out = np.zeros(inv.shape[:-1] + (K,), dtype=np.int32)
    out[..., :inv.shape[-1]] = inv
    return out
