"""The five entry points of the device-resident L-BFGS at the C ABI, no device: declared in the header, exported by the library, bound
in the ctypes table with the header's argument types, outside the setter / bind name patterns, and refusing a null handle.  Everything
that needs an engine: tests/test_gpu_lbfgs.py."""
import ctypes as C
import os
import re

import gpe_pinn
from gpe_pinn import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpe_lbfgs_config", "gpe_lbfgs_update", "gpe_lbfgs_run", "gpe_lbfgs_read", "gpe_lbfgs_history")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpe_hip.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_bound():
    code = _code()
    assert re.search(r"int\s+gpe_lbfgs_config\s*\(\s*gpe_engine\s*\*\s*e\s*,\s*double\s+lr\s*,\s*int\s+history\s*,\s*double\s+tolerance_grad\s*,"
                     r"\s*double\s+tolerance_change\s*,\s*double\s+stop_loss\s*\)\s*;", code)
    assert re.search(r"int\s+gpe_lbfgs_update\s*\(\s*gpe_engine\s*\*\s*e\s*\)\s*;", code)
    assert re.search(r"int\s+gpe_lbfgs_run\s*\(\s*gpe_engine\s*\*\s*e\s*,\s*int64_t\s+n_iters\s*,\s*int\s+mse\s*\)\s*;", code)
    assert re.search(r"int\s+gpe_lbfgs_read\s*\(\s*gpe_engine\s*\*\s*e\s*,\s*double\s+out\[16\]\s*\)\s*;", code)
    assert re.search(r"int\s+gpe_lbfgs_history\s*\(\s*gpe_engine\s*\*\s*e\s*,\s*float\s*\*\s*h_S\s*,\s*float\s*\*\s*h_Y\s*,\s*float\s*\*\s*h_g_prev\s*,"
                     r"\s*float\s*\*\s*h_d\s*,\s*size_t\s+n\s*,\s*int\s*\*\s*count\s*\)\s*;", code)
    lib = C.CDLL(capi.library_path())
    for name in NEW:
        assert hasattr(lib, name), f"{name} not exported"
    vp, dbl = C.c_void_p, C.c_double
    assert capi.SYMBOLS["gpe_lbfgs_config"] == (C.c_int, [vp, dbl, C.c_int, dbl, dbl, dbl])
    assert capi.SYMBOLS["gpe_lbfgs_update"] == (C.c_int, [vp])
    assert capi.SYMBOLS["gpe_lbfgs_run"] == (C.c_int, [vp, C.c_int64, C.c_int])
    assert capi.SYMBOLS["gpe_lbfgs_read"] == (C.c_int, [vp, C.POINTER(dbl)])
    assert capi.SYMBOLS["gpe_lbfgs_history"] == (C.c_int, [vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_int)])
    declared = sorted(set(re.findall(r"\b(gpe_[a-z0-9_]+)\s*\(", code)))
    assert sorted(capi.SYMBOLS) == declared, "ctypes table and header disagree"


def test_the_names_stay_outside_the_setter_and_bind_pattern_and_no_switch_was_added():
    for name in NEW:
        assert not re.match(r"gpe_(set|bind)_", name)
    for f in ("gpe_lbfgs.h", "gpe_lbfgs_rules.h"):
        assert "getenv" not in open(os.path.join(ROOT, "gross-pitaevskii-eigenvalue-problem_amd", "csrc", f)).read()


def test_a_null_engine_is_refused():
    lib = capi.load()
    out = (C.c_double * 16)()
    n = C.c_int()
    assert lib.gpe_lbfgs_config(None, 0.1, 10, 1e-7, 1e-9, 0.0) == capi.GPE_ERR_INVALID
    assert lib.gpe_lbfgs_update(None) == capi.GPE_ERR_INVALID
    assert lib.gpe_lbfgs_run(None, 1, 0) == capi.GPE_ERR_INVALID
    assert lib.gpe_lbfgs_read(None, out) == capi.GPE_ERR_INVALID
    assert lib.gpe_lbfgs_history(None, None, None, None, None, 0, C.byref(n)) == capi.GPE_ERR_INVALID


def test_the_python_surface():
    for name in ("lbfgs_config", "lbfgs_update", "lbfgs_run", "lbfgs_read", "lbfgs_history"):
        assert callable(getattr(gpe_pinn.Engine, name))
    assert gpe_pinn.Engine.LBFGS_FIELDS[:4] == ("loss", "grad_max", "grad_l1", "t") and len(gpe_pinn.Engine.LBFGS_FIELDS) <= 16
    import inspect
    from gpe_pinn import refine
    assert inspect.signature(refine.pretrain_on_analytical_solution).parameters["lbfgs"].default == "host"
