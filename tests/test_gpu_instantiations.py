"""GPU: one cell per pair-kernel instantiation of the launch record (util.INST_CELLS; tests/test_instantiations.py checks on
the CPU that the cells cover the table and lead the dispatch there).  Every cell clears the LZANI_* switches, sets its own,
runs its call and asserts (tests/inst_cell.py: run_cell) that
- the launch record names exactly the cell's kernel (a split cell: both modes of its k_split) and no other pair kernel;
- the results are bit-equal to the oracle (the matching entries of its all2all for query lists);
- regions cells: every region of every pair equals O.oracle_pair(..., want_regions=True);
- run-time compiled cells: no compile failed, and rtc_info() reports the null chain as chain_params_ok says."""
import pytest

import util as U
from inst_cell import oracle_of, run_cell

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtc_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rtc_cache"))


@pytest.mark.parametrize("cell", U.INST_CELLS, ids=[c["id"] for c in U.INST_CELLS])
def test_instantiation_matches_the_oracle(monkeypatch, rtc_cache, cell):
    run_cell(monkeypatch, rtc_cache, cell, U.instantiation_set(cell["set"]), oracle_of(cell["set"], cell["prm"]))
