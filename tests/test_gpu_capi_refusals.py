"""GPU: what the entries that take a ``mpcasm_plan*`` refuse, row by row (refusal_cases.GPU_ROWS), on three
assemblers at batch 2.  Every row is decided before any device work -- a negative status, or the MPCASM_OK of an
empty call -- and the results, filled with NaN beforehand, are still NaN once the device is idle.  The table is held
to what the library answered before the entries shared their opening lines (profiles/capi_refusals.txt), and the
library to the table.  The rows with another device current need two devices and are skipped on one; among them
``mpcasm_preview_matrices`` is the one status that changed: it used to launch there."""
import pytest

import refusal_cases as rc
from mpcasm import capi

pytestmark = pytest.mark.gpu
ENTRIES = sorted({row.entry for row in rc.GPU_ROWS})
_bench = []


@pytest.fixture
def bench(gpu_api):
    if not _bench:
        _bench.append(rc.GpuBench(gpu_api))
    return _bench[0]


def test_the_table_is_what_was_recorded():
    assert [rc.line("gpu", row, row.code, row.out) for row in rc.GPU_ROWS if row.recorded] == rc.recorded("gpu")
    # not recorded: the rows that need a second device, nothing else
    assert {row.variant for row in rc.GPU_ROWS if not row.recorded} == {"wrong device"}
    assert sorted(row.entry for row in rc.GPU_ROWS if row.variant == "wrong device") == sorted(rc.GPU_ARGS)


def test_the_table_covers_every_entry_that_takes_a_plan():
    assert ENTRIES == sorted(rc.GPU_ARGS)
    assert len({(row.entry, row.plan, row.variant) for row in rc.GPU_ROWS}) == len(rc.GPU_ROWS)
    for entry in ENTRIES:
        variants = {row.variant for row in rc.GPU_ROWS if row.entry == entry}
        assert "null plan" in variants and variants & {"batch=-1", "count=-1"}, entry
        assert entry == "mpcasm_plan_prepare" or variants & {"batch=0", "count=0"}, entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_library_answers_as_the_table_says(bench, entry):
    lib = capi.load()
    for row in rc.GPU_ROWS:
        if row.entry == entry and row.variant != "wrong device":
            code = bench.run(lib, row)
            assert code == row.code, rc.line("gpu", row, code, rc.NO_OUT)
    assert bench.results_untouched()


def test_another_device_current_is_refused_by_every_entry(bench):
    lib = capi.load()
    if lib.mpcasm_device_count() < 2:
        pytest.skip("one device: no other one to make current")
    for row in rc.GPU_ROWS:
        if row.variant == "wrong device":
            code = bench.run(lib, row)
            assert code == row.code == rc.ARG, rc.line("gpu", row, code, rc.NO_OUT)
    assert bench.results_untouched()
