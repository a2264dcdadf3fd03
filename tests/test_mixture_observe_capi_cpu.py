"""The mixture observables, monitor and keeper at the C ABI, no device: the six entry points are declared, exported and bound with the
argument types the header states, the ctypes record has the library's size and at most 64 doubles (the keeper files one per lane of a
wave), and no new declaration is a gpe_set_* / gpe_bind_* (tests/live_table.py lists those)."""
import ctypes as C
import os
import re

from gpe_pinn import Engine, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = C.POINTER(capi.gpe_mixture_observables)
ENTRY_POINTS = {
    "gpe_sizeof_mixture_observables": (C.c_size_t, []),
    "gpe_mixture_observables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, REC]),
    "gpe_mixture_monitor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_int64, C.c_int32]),
    "gpe_mixture_monitor_read": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, REC, C.POINTER(C.c_int64)]),
    "gpe_mixture_keeper": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int64]),
    "gpe_mixture_keeper_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, REC, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
}


def _header():
    txt = open(os.path.join(ROOT, "include", "gpe_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_declared_exported_and_bound_with_the_headers_argument_counts():
    txt = _header()
    lib = C.CDLL(capi.library_path())
    for name, (res, args) in ENTRY_POINTS.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} not declared in include/gpe_hip.h"
        declared = [a for a in m.group(1).split(",") if a.strip() not in ("", "void")]
        assert len(declared) == len(args), (name, declared)
        assert hasattr(lib, name), f"{name} not exported"
        assert capi.SYMBOLS[name] == (res, args), name
    assert re.search(r"struct\s+gpe_mixture_observables\s*\{", txt)
    assert "#define GPE_ABI_VERSION 2" in txt and capi.GPE_ABI_VERSION == 2


def test_record_size_matches_the_library_and_fits_one_wave():
    lib = C.CDLL(capi.library_path())
    lib.gpe_sizeof_mixture_observables.restype = C.c_size_t
    size = C.sizeof(capi.gpe_mixture_observables)
    assert lib.gpe_sizeof_mixture_observables() == size == 8 * len(Engine.MIXTURE_OBSERVABLE_FIELDS)
    assert size % 8 == 0 and size // 8 <= 64
    body = re.search(r"struct\s+gpe_mixture_observables\s*\{(.*?)\};", _header(), re.S).group(1)
    assert not re.search(r"\b(float|int|int32_t|int64_t|char|long)\b", body), "the record is all doubles"
    d = capi.gpe_mixture_observables().as_dict()
    assert list(d)[:4] == ["n", "dv", "step", "norm"] and len(d["inter"]) == 3 and [len(r) for r in d["mean_x"]] == [3, 3]
    assert Engine.MIXTURE_OBSERVABLE_FIELDS.index("energy") == capi.gpe_mixture_observables.energy.offset // 8
    assert Engine.MIXTURE_OBSERVABLE_FIELDS.index("res_rms_total") == capi.gpe_mixture_observables.res_rms_total.offset // 8 == size // 8 - 1


def test_no_new_setter_or_binder_and_a_null_engine_is_refused():
    assert not [n for n in ENTRY_POINTS if n.startswith(("gpe_set_", "gpe_bind_"))]
    lib = capi.load()
    rec = capi.gpe_mixture_observables()
    assert lib.gpe_mixture_observables(None, None, 0, None, 1.0, C.byref(rec)) == capi.GPE_ERR_INVALID
    assert lib.gpe_mixture_monitor(None, None, 0, None, 1.0, 1, 0) == capi.GPE_ERR_INVALID
    assert lib.gpe_mixture_monitor_read(None, 0, 0, None, None) == capi.GPE_ERR_INVALID
    assert lib.gpe_mixture_keeper(None, capi.KEEP_RES_RMS, 0.0, 0) == capi.GPE_ERR_INVALID
    assert lib.gpe_mixture_keeper_read(None, None, 0, None, None, None, None, None) == capi.GPE_ERR_INVALID


def test_engine_exposes_the_methods():
    for name in ("mixture_observables", "bind_mixture_monitor", "read_mixture_monitor", "read_mixture_monitor_array", "bind_mixture_keeper",
                 "keeper_state", "best_params", "best_record", "restore_best"):
        assert callable(getattr(Engine, name)), name
