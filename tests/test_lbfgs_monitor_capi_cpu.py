"""The two entry points that put the device-resident L-BFGS under the held-out monitor and the keeper, at the C ABI, no device: declared in
the header, exported by the library, bound in the ctypes table with the header's argument types, outside the setter / bind name patterns,
refusing a null handle; frozen code 4 and the Python surface.  Everything that needs an engine: tests/test_gpu_lbfgs_monitor.py."""
import ctypes as C
import inspect
import os
import re

import gpe_pinn
from gpe_pinn import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gross-pitaevskii-eigenvalue-problem_amd", "csrc")
NEW = ("gpe_lbfgs_monitor", "gpe_lbfgs_point")


def _header():
    return open(os.path.join(ROOT, "include", "gpe_hip.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def test_symbols_are_declared_exported_and_bound():
    code = _code()
    assert re.search(r"int\s+gpe_lbfgs_monitor\s*\(\s*gpe_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", code)
    assert re.search(r"int\s+gpe_lbfgs_point\s*\(\s*gpe_engine\s*\*\s*e\s*,\s*float\s*\*\s*h_flat\s*,\s*size_t\s+n\s*\)\s*;", code)
    lib = C.CDLL(capi.library_path())
    for name in NEW:
        assert hasattr(lib, name), f"{name} not exported"
        assert not re.match(r"gpe_(set|bind)_", name)
    assert capi.SYMBOLS["gpe_lbfgs_monitor"] == (C.c_int, [C.c_void_p, C.c_int])
    assert capi.SYMBOLS["gpe_lbfgs_point"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t])
    declared = sorted(set(re.findall(r"\b(gpe_[a-z0-9_]+)\s*\(", code)))
    assert sorted(capi.SYMBOLS) == declared, "ctypes table and header disagree"


def test_a_null_engine_is_refused_and_no_switch_was_added():
    lib = capi.load()
    buf = (C.c_float * 4)()
    assert lib.gpe_lbfgs_monitor(None, 1) == capi.GPE_ERR_INVALID
    assert lib.gpe_lbfgs_point(None, buf, 4) == capi.GPE_ERR_INVALID
    for f in ("gpe_lbfgs.h", "gpe_lbfgs_rules.h"):
        assert "getenv" not in open(os.path.join(CSRC, f)).read()


def test_the_header_states_the_rule_and_the_code():
    text = _header()
    assert "NOT served" not in text
    run = text[text.index(" * gpe_lbfgs_run:"):text.index(" * gpe_lbfgs_read:")]
    assert "gpe_lbfgs_monitor" in run and "start" in run and "trial" in run           # the judged point, stated where the run is
    assert re.search(r"4 the keeper", text[text.index(" * gpe_lbfgs_read:"):text.index(" * gpe_lbfgs_history:")])
    assert re.search(r"LBFGS_FROZEN_KEEPER\s*=\s*4\b", open(os.path.join(CSRC, "gpe_lbfgs_rules.h")).read())


def test_frozen_code_4_and_the_python_surface():
    E = gpe_pinn.Engine
    assert E.LBFGS_FROZEN[4] == "keeper" and len(E.LBFGS_FROZEN) == 5
    assert "keeper" in E.lbfgs_read.__doc__ and "4" in E.lbfgs_read.__doc__
    assert inspect.signature(E.lbfgs_monitor).parameters["on"].default is True
    assert list(inspect.signature(E.lbfgs_point).parameters) == ["self"]
    assert "not served" not in E.lbfgs_run.__doc__
    from gpe_pinn import surface
    p = inspect.signature(surface._refine_pretrain).parameters
    assert p["lbfgs_monitor"].default is False and p["lbfgs"].default == "host" and p["lbfgs_line_search"].default is None
    from gpe_pinn import refine
    assert inspect.signature(refine.pretrain_on_analytical_solution).parameters["lbfgs_monitor"].default is False
