"""Shared test helpers: compiled configs for the worlds the fixtures use."""
import numpy as np

from psketch_amd import gamedef
from psketch_amd.cookbook import Cookbook, TaskManager, compile_config, world_params


def make_tables(world="craft_medium", max_timesteps=gamedef.MAX_TIMESTEPS):
    params = world_params(world)
    cb = Cookbook()
    tm = TaskManager()
    cfg = compile_config(params, cb, tm, max_timesteps)
    return params, cb, tm, cfg


def world_for(W, window):
    name = {(8, 3): "craft_medium", (12, 3): "craft_medium_12x12",
            (12, 5): "craft_medium_12x12_w5", (10, 5): "craft_large"}[(W, window)]
    return name


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
