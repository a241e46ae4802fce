"""CPU: what the twelve host-only queries of the C boundary refuse, row by row (refusal_cases.CPU_ROWS): the status,
and whether the caller's results are left as they were (every MPCASM_ERR_ARG) or zeroed (every later refusal).  The
table is held to what the library answered before the entries shared their opening lines
(profiles/capi_refusals.txt), and the library to the table: integer codes and bit patterns, no tolerance."""
import pytest

import refusal_cases as rc
from mpcasm import capi

ENTRIES = sorted({row.entry for row in rc.CPU_ROWS})
_plans = {}


@pytest.fixture
def plans(cpu_api):
    if not _plans:
        _plans.update(rc.cpu_plans(cpu_api))
    return _plans


def test_the_table_is_what_was_recorded():
    assert [rc.line("cpu", row, row.code, row.out) for row in rc.CPU_ROWS if row.recorded] == rc.recorded("cpu")
    assert all(row.recorded for row in rc.CPU_ROWS)


def test_the_table_covers_the_twelve_queries():
    assert len(ENTRIES) == 12 and len(rc.CPU_ROWS) >= 100
    assert len({(row.entry, row.plan, row.variant) for row in rc.CPU_ROWS}) == len(rc.CPU_ROWS)
    for entry in ENTRIES:          # the table pointers and the truncated tables, for every one of them
        variants = {row.variant for row in rc.CPU_ROWS if row.entry == entry}
        assert {"null h_itab", "null h_dtab", "truncated"} <= variants, entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_library_answers_as_the_table_says(plans, entry):
    lib = capi.load()
    for row in rc.CPU_ROWS:
        if row.entry == entry:
            code, out = rc.run_cpu_row(lib, plans, row)
            assert (code, out) == (row.code, row.out), rc.line("cpu", row, code, out)
