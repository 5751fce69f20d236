"""bench.py's plain run and --dump-outputs on the card: one small run (2,048 envs, 5 warmup and
20 timed ticks) prints a line without the --full blocks, times exactly --steps ticks, and the
arrays it dumps are the last timed tick's outputs, bit-exact against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, POOL, WARMUP, STEPS = 2048, 64, 5, 20


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                          "--warmup", str(WARMUP), "--envs", str(N), "--pool", str(POOL),
                          "--dump-outputs", str(d)], cwd=REPO, env=env, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), d


def test_plain_line_has_the_headline_and_nothing_that_takes_runs_of_its_own(plain_run):
    line, _ = plain_run
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N * 1e3 / line["ms_per_step"])
    assert "roofline" not in line and "cpu_baseline" not in line
    # exactly the warmup and the timed ticks ran: no launch besides them
    assert line["episodes"]["env_steps"] == N * (WARMUP + STEPS)


def test_dumped_outputs_are_the_last_timed_tick(plain_run, oracle_mod):
    _, d = plain_run
    from psketch_amd.sim import sample_scenarios, synthetic_specs
    from tests.helpers import make_tables
    params, cb, tm, cfg = make_tables("craft_medium_12x12")
    grids, _, _ = sample_scenarios(params, cb, 123, POOL)
    specs = synthetic_specs(grids, 12, 12, N, 0, seed=0, task_ids=[t.id for t in tm.dataset_tasks()])
    o = oracle_mod.Oracle(cfg, grids)
    envs = o.init_envs(*specs)
    for t in range(WARMUP + STEPS):
        rc, obs, reward, done, success = o.batch_tick(envs, 0, None, 0, t, True, want_obs=t == WARMUP + STEPS - 1)
        assert rc == 0
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert sorted(got) == ["done", "obs", "obs_rows", "reward", "success"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["obs_rows"].tolist() == list(range(N))           # 2,048 rows fit: every env
    assert np.array_equal(got["obs"], obs)
    assert np.array_equal(got["reward"], reward)
    assert np.array_equal(got["done"], done)
    assert np.array_equal(got["success"], success)
    assert done.any() or obs.any()
