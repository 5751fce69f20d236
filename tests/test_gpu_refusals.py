"""The refusal table (tests/refusal_cases.py) on the HIP library and the CPU variant side by side:
status and text equal row by row, each equal to the table's, and the HIP handle unchanged.  Every
row is refused before any launch."""
import pytest

from tests.refusal_cases import ROWS, check_row, check_valid_tick, make_handles, refuse

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles(gpu):
    return make_handles(gpu.index), make_handles("cpu")


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_refused_hip_as_cpu(handles, row):
    hip, cpu = handles
    check_row(hip[row.handle], row)
    assert refuse(hip[row.handle], row) == refuse(cpu[row.handle], row)


def test_refused_tune_leaves_the_rollout_shape(gpu):
    """craft_sim_tune(48, ...) is refused and the handle keeps its tile: at a 5x5 window the
    rollout would otherwise resolve to a 48-env tile no kernel is instantiated for.  Read off the
    shape queries only."""
    c = make_handles(gpu.index, ("w5",))["w5"]
    before = c.sim.rollout_shape(), c.sim.tile_shape()
    status, _ = refuse(c, next(r for r in ROWS if r.id == "tune-tile48"))
    assert status != 0
    assert (c.sim.rollout_shape(), c.sim.tile_shape()) == before
    assert c.sim.rollout_shape()[0] in (16, 32, 64)


def test_valid_tick_after_every_refusal_hip(gpu, oracle_mod):
    handles = make_handles(gpu.index)
    for row in ROWS:
        status, _ = refuse(handles[row.handle], row)
        assert status == row.status, row.id
    check_valid_tick(handles["base"], oracle_mod)
