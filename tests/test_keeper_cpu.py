"""gpe_pinn/keeper.py:select -- the keeper's rule in plain Python, the reference of tests/test_gpu_keeper.py -- on hand-made sequences,
and the three keeper entry points in the ctypes table with the argument types include/gpe_hip.h declares."""
import ctypes as C
import math
import os
import re

import pytest

from gpe_pinn import capi, keeper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = math.nan, math.inf


def test_strictly_falling_keeps_every_record_and_the_last_at_the_end():
    assert keeper.select([5.0, 4.0, 3.0, 2.5]) == (3, [0, 1, 2, 3], None)
    assert keeper.select([5.0, 4.0, 3.0, 2.5], patience=1) == (3, [0, 1, 2, 3], None)
    assert keeper.counters(4, [0, 1, 2, 3]) == dict(seen=4, kept=4, since_best=0)


def test_falling_then_rising_keeps_the_minimum_and_stops_patience_records_later():
    v = [5.0, 3.0, 1.0, 2.0, 4.0, 8.0, 16.0]
    assert keeper.select(v) == (2, [0, 1, 2], None)
    assert keeper.select(v, patience=3) == (2, [0, 1, 2], 5)
    assert keeper.select(v, patience=4) == (2, [0, 1, 2], 6)
    assert keeper.select(v, patience=5) == (2, [0, 1, 2], None)
    assert keeper.counters(len(v), [0, 1, 2]) == dict(seen=7, kept=3, since_best=4)
    # a later, lower minimum behind the stop is still reported as kept: select, like the device, judges every value it is given
    assert keeper.select(v + [0.5], patience=3) == (7, [0, 1, 2, 7], 5)


def test_a_tie_is_no_improvement():
    assert keeper.select([2.0, 2.0, 2.0]) == (0, [0], None)
    assert keeper.select([2.0, 2.0, 2.0], patience=2) == (0, [0], 2)
    assert keeper.select([2.0, 1.0, 1.0, 1.0 - 2.0 ** -52]) == (3, [0, 1, 3], None)


def test_a_gain_smaller_than_min_delta_is_not_kept():
    v = [1.0, 0.95, 0.85, 0.84, 0.70]
    assert keeper.select(v, min_delta=0.1) == (4, [0, 2, 4], None)          # 0.95: gain 0.05; 0.84: gain 0.01 on the kept 0.85
    assert keeper.select(v, min_delta=0.2) == (4, [0, 4], None)             # gains are measured from the KEPT value, not the last one
    assert keeper.select([1.0, 0.9], min_delta=0.1) == (0, [0], None)       # m < best - min_delta is strict (1.0 - 0.1 = 0.9 exactly)
    assert keeper.select(v, min_delta=0.1, patience=1) == (4, [0, 2, 4], 1)


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_non_finite_values_are_never_kept(bad):
    assert keeper.select([bad, 3.0, 2.0]) == (2, [1, 2], None)                # first: the first finite value is the first kept
    assert keeper.select([3.0, bad, 2.0]) == (2, [0, 2], None)                # in the middle: counted as no improvement
    assert keeper.select([3.0, bad, bad, 2.0], patience=2) == (3, [0, 3], 2)
    assert keeper.select([bad, bad, bad]) == (None, [], None)                 # nothing kept, and no stop without patience
    assert keeper.select([bad, bad, bad], patience=3) == (None, [], 2)        # patience counts from the start
    assert keeper.counters(3, []) == dict(seen=3, kept=0, since_best=3)


def test_patience_one_stops_at_the_first_record_without_improvement():
    assert keeper.select([3.0, 2.0, 2.5, 1.0], patience=1) == (3, [0, 1, 3], 2)
    assert keeper.select([3.0, 3.0], patience=1) == (0, [0], 1)
    assert keeper.select([], patience=1) == (None, [], None)


def test_select_refuses_what_the_engine_refuses():
    for kw in (dict(min_delta=-1e-9), dict(min_delta=NAN), dict(min_delta=INF), dict(patience=-1)):
        with pytest.raises(ValueError):
            keeper.select([1.0], **kw)


def test_select_takes_numpy_float32_and_compares_in_float64():
    import numpy as np
    v = np.array([1.0, 1.0 - 2.0 ** -24], np.float32)                         # two neighbouring floats: an improvement, if a small one
    assert keeper.select(v) == (1, [0, 1], None)
    assert keeper.select(v, min_delta=2.0 ** -24) == (0, [0], None)            # exactly the gain: strict comparison in float64


def _declaration(name):
    txt = open(os.path.join(ROOT, "include", "gpe_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} not declared in include/gpe_hip.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


C_TYPES = {"gpe_engine*": C.c_void_p, "float*": C.c_void_p, "int": C.c_int, "double": C.c_double, "int64_t": C.c_int64, "size_t": C.c_size_t,
           "struct gpe_observables*": C.POINTER(capi.gpe_observables), "int64_t*": C.POINTER(C.c_int64), "int*": C.POINTER(C.c_int)}


@pytest.mark.parametrize("name", ["gpe_bind_keeper", "gpe_keeper_read", "gpe_keeper_restore"])
def test_keeper_symbols_carry_the_headers_argument_types(name):
    assert name in capi.SYMBOLS
    res, args = capi.SYMBOLS[name]
    assert res is C.c_int
    declared = [C_TYPES[a.rsplit(" ", 1)[0].replace("const ", "")] for a in _declaration(name)]       # "type name" -> type
    assert args == declared, (name, args, declared)


def test_metric_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "gpe_hip.h")).read()
    for nm in ("NONE", "RES_RMS", "ENERGY"):
        m = re.search(r"GPE_KEEP_" + nm + r"\s*=\s*(\d+)", txt)
        assert m and int(m.group(1)) == getattr(capi, "KEEP_" + nm)
    assert keeper.METRICS == ("res_rms", "energy")
