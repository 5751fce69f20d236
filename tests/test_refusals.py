"""Every refusal of the shared argument checks (psketch_amd/csrc/craft_checks.h) on the CPU variant
of the ABI: status and text as tests/refusal_cases.py records them, the handle unchanged, and a
valid tick afterwards still the oracle's.  tests/test_gpu_refusals.py runs the same table on the
HIP library."""
import os
import re

import pytest

from tests.refusal_cases import ROWS, check_row, check_valid_tick, make_handles, refuse

CHECKS_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "psketch_amd", "csrc",
                        "craft_checks.h")


@pytest.fixture(scope="module")
def handles():
    return make_handles("cpu")


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_refused_cpu(handles, row):
    check_row(handles[row.handle], row)


def test_valid_tick_after_every_refusal_cpu(oracle_mod):
    handles = make_handles("cpu")
    for row in ROWS:
        status, _ = refuse(handles[row.handle], row)
        assert status == row.status, row.id
    for name in ("base", "w5"):
        check_valid_tick(handles[name], oracle_mod)


def test_every_message_of_the_shared_header_has_a_row():
    """Every string literal of craft_checks.h (whole messages, and the pieces of the three built
    ones) occurs in the expected text of some row."""
    with open(CHECKS_H) as f:
        src = "\n".join(line for line in f.read().splitlines() if not line.lstrip().startswith(("#", "//")))
    literals = [m.encode().decode("unicode_escape") for m in re.findall(r'"((?:[^"\\]|\\.)*)"', src)]
    assert len(literals) >= 60, "the message literals were not found"
    texts = [r.message for r in ROWS]
    missing = [lit for lit in literals if not any(lit in t for t in texts)]
    assert not missing, missing
    # the whole messages (they name their entry point) are hit exactly, not as a substring
    whole = [lit for lit in literals if re.match(r"craft_\w+: ", lit) and not lit.endswith(" ")]
    assert not [lit for lit in whole if lit not in texts]
