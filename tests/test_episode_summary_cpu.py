"""craft_episode_summary on the CPU variant (CraftSim(device="cpu")): the shared cases of
tests/episode_summary_cases.py against the copy of the host loop it replaces and against the
oracle, and the refusals of tests/episode_summary_refusal_cases.py."""
import pytest

from tests import episode_summary_cases as C
from tests import episode_summary_refusal_cases as RC
from tests.refusal_cases import check_row, make_handles


@pytest.mark.parametrize("lang", [False, True], ids=["step_stream", "step_lang_stream"])
def test_dev_split_table_on_and_off_cpu(golden, oracle_mod, lang):
    C.check_dev_split(golden, oracle_mod, "cpu", lang)


@pytest.mark.parametrize("n,rows,ticks", [(70, None, None), (20, 7, None), (70, None, 1)],
                         ids=["70_slots", "20_slots_7_rows", "one_tick"])
def test_slot_counts_cpu(oracle_mod, n, rows, ticks):
    C.check_slot_counts(oracle_mod, "cpu", n, rows=rows, ticks=ticks)


def test_every_slot_stops_every_tick_cpu(oracle_mod):
    C.check_every_slot_stops_every_tick(oracle_mod, "cpu")


def test_records_without_an_end_cpu():
    C.check_no_end("cpu")


@pytest.mark.parametrize("mode", ["hashed", "label"])
def test_chunks_with_carry_cpu(oracle_mod, mode):
    C.check_chunks(oracle_mod, "cpu", mode)


@pytest.mark.parametrize("tag", [C.RECT_SMALLEST, C.RECT_LARGEST])
def test_rectangular_worlds_cpu(oracle_mod, tag):
    C.check_rect(oracle_mod, "cpu", tag)


def test_flags_and_latches_cpu(golden, oracle_mod):
    C.check_flags(golden, oracle_mod, "cpu")


def test_handle_left_alone_cpu():
    C.check_handle_left_alone("cpu")


@pytest.mark.parametrize("lang", [False, True], ids=["evaluate", "language_evaluate"])
def test_evaluate_leaves_the_handle_cpu(golden, lang):
    C.check_evaluate_leaves_the_handle(golden, "cpu", lang)


def test_replay_reports_distances_cpu(golden, oracle_mod):
    C.check_replay_distances(golden, oracle_mod, "cpu")


@pytest.fixture(scope="module")
def handles():
    return make_handles("cpu", names=RC.HANDLES)


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_episode_summary_refuses_cpu(handles, row):
    check_row(handles[row.handle], row)


def test_episode_summary_accepts_cpu(handles):
    RC.check_accepts(handles["queued"])
