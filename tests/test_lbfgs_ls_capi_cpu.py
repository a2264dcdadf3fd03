"""The two entry points of the strong-Wolfe line search at the C ABI, no device: declared in the header, exported by the library, bound in
the ctypes table with the header's argument types, outside the setter / bind name patterns, refusing a null handle; the Python surface.
Everything that needs an engine (the argument checks included: they come behind the handle): tests/test_gpu_lbfgs_ls.py."""
import ctypes as C
import inspect
import os
import re

import gpe_pinn
from gpe_pinn import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpe_lbfgs_line_search", "gpe_lbfgs_ls_read")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpe_hip.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_bound():
    code = _code()
    assert re.search(r"int\s+gpe_lbfgs_line_search\s*\(\s*gpe_engine\s*\*\s*e\s*,\s*int\s+kind\s*,\s*double\s+c1\s*,\s*double\s+c2\s*,\s*int\s+max_ls\s*\)\s*;",
                     code)
    assert re.search(r"int\s+gpe_lbfgs_ls_read\s*\(\s*gpe_engine\s*\*\s*e\s*,\s*double\s+out\[24\]\s*\)\s*;", code)
    lib = C.CDLL(capi.library_path())
    for name in NEW:
        assert hasattr(lib, name), f"{name} not exported"
        assert not re.match(r"gpe_(set|bind)_", name)
    assert capi.SYMBOLS["gpe_lbfgs_line_search"] == (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int])
    assert capi.SYMBOLS["gpe_lbfgs_ls_read"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_double)])
    declared = sorted(set(re.findall(r"\b(gpe_[a-z0-9_]+)\s*\(", code)))
    assert sorted(capi.SYMBOLS) == declared, "ctypes table and header disagree"


def test_a_null_engine_is_refused_and_no_switch_was_added():
    lib = capi.load()
    out = (C.c_double * 24)()
    assert lib.gpe_lbfgs_line_search(None, 1, 1e-4, 0.9, 25) == capi.GPE_ERR_INVALID
    assert lib.gpe_lbfgs_ls_read(None, out) == capi.GPE_ERR_INVALID
    for f in ("gpe_lbfgs.h", "gpe_lbfgs_rules.h"):
        assert "getenv" not in open(os.path.join(ROOT, "gross-pitaevskii-eigenvalue-problem_amd", "csrc", f)).read()


def test_the_record_and_the_python_surface():
    E = gpe_pinn.Engine
    assert len(E.LBFGS_LS_FIELDS) == 24 and len(set(E.LBFGS_LS_FIELDS)) == 24
    m = re.search(r"LSR_PHASE = 0,(.*?)LSR_FIELDS = (\d+)", open(os.path.join(ROOT, "gross-pitaevskii-eigenvalue-problem_amd", "csrc", "gpe_lbfgs_rules.h")).read(),
                  re.S)
    assert int(m.group(2)) == len(E.LBFGS_LS_FIELDS) and m.group(1).count("LSR_") == len(E.LBFGS_LS_FIELDS) - 1
    assert callable(E.lbfgs_ls_read)
    p = inspect.signature(E.lbfgs_config).parameters
    assert p["line_search"].default is None and p["c1"].default == 1e-4 and p["c2"].default == 0.9 and p["max_ls"].default == 25
    from gpe_pinn import refine
    assert inspect.signature(refine.pretrain_on_analytical_solution).parameters["lbfgs_line_search"].default is None
