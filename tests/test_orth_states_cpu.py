"""CPU-side check of the frozen-orthogonality-state entry points: the ctypes table carries both, with as many arguments as
include/gpe_hip.h declares, and the Engine exposes them."""
import os
import re

import gpe_pinn
from gpe_pinn import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_arg_count(name):
    txt = open(os.path.join(ROOT, "include", "gpe_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} not declared in include/gpe_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_capi_table_carries_the_orth_state_entry_points():
    for name, want in (("gpe_bind_orth_state", 7), ("gpe_orth_values", 4)):
        assert name in capi.SYMBOLS, f"{name} missing from the ctypes table"
        res, args = capi.SYMBOLS[name]
        assert _declared_arg_count(name) == want
        assert len(args) == want and res is capi.C.c_int
    assert callable(gpe_pinn.Engine.bind_orth_state) and callable(gpe_pinn.Engine.orth_values)
