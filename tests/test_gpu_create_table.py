"""Engine creation decides the same as the commit named in tests/golden/create_table.json did: path, parameter count and the
active_kernels strings of every cell of tests/create_table.py (each class of the switch matrix under the default environment and under
every switch value that applies to it), compared for exact equality.  Engines are created and strings read; no step runs.  A class or
a switch value added to the tables fails here until the golden is regenerated (tools/create_table.py)."""
import json
import os

import pytest

from tests import create_table as CT
from tests import test_gpu_switch_matrix as M

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_table.json")) as _f:
    GOLDEN = json.load(_f)
CELLS = CT.cells()


def test_the_golden_holds_the_cells_of_the_tables_and_no_others():
    assert GOLDEN["parent"] and len(CELLS) >= 300
    assert sorted(GOLDEN["cells"]) == sorted(CELLS), (sorted(set(CELLS) - set(GOLDEN["cells"])), sorted(set(GOLDEN["cells"]) - set(CELLS)))


@pytest.mark.parametrize("name,bi", M.CELLS, ids=[f"{n}-{b}" for n, b in M.CELLS])
def test_creation_decides_what_the_parent_decided(name, bi):
    mine = {k: c for k, c in CELLS.items() if c[:2] == (name, bi)}
    assert mine
    bad = []
    for k, c in mine.items():
        got, want = CT.record(*c), GOLDEN["cells"].get(k)
        if got != want:
            bad.append(f"{k}: {got} != {want} (commit {GOLDEN['parent']})")
    assert not bad, f"{len(bad)} of {len(mine)} cells differ\n" + "\n".join(bad)
