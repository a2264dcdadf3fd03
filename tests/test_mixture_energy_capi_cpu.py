"""The two entry points of the mixture energy term (gpe_mixture_energy_weight, gpe_mixture_energy) at the C ABI, no device: declared in
the header, exported by the library, bound in the ctypes table with the header's argument types; gpe_config unchanged (the weight is
engine state, not configuration); and the refusals that need no engine -- a null handle, and w_riesz in a mixture configuration, which
stays refused at gpe_create (the scalar Riesz term is not the mixture's energy).  The refusal on a live non-mixture engine needs a device:
tests/test_gpu_mixture_energy.py."""
import ctypes as C
import os
import re

import gpe_pinn
from gpe_pinn import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpe_mixture_energy_weight", "gpe_mixture_energy")


def _header():
    return open(os.path.join(ROOT, "include", "gpe_hip.h")).read()


def test_both_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+gpe_mixture_energy_weight\s*\(\s*gpe_engine\s*\*\s*e\s*,\s*float\s+w_E\s*\)\s*;", code)
    assert re.search(r"int\s+gpe_mixture_energy\s*\(\s*gpe_engine\s*\*\s*e\s*,\s*double\s+out\[8\]\s*\)\s*;", code)
    lib = C.CDLL(capi.library_path())
    for name in NEW:
        assert hasattr(lib, name), f"{name} not exported"
    assert capi.SYMBOLS["gpe_mixture_energy_weight"] == (C.c_int, [C.c_void_p, C.c_float])
    assert capi.SYMBOLS["gpe_mixture_energy"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_double)])
    declared = sorted(set(re.findall(r"\b(gpe_[a-z0-9_]+)\s*\(", code)))
    assert sorted(capi.SYMBOLS) == declared, "ctypes table and header disagree"


def test_the_names_stay_outside_the_setter_and_bind_pattern():
    """tests/live_table.py lists every gpe_set_* / gpe_bind_* of the header; the weight's live-engine test is its own
    (tests/test_gpu_mixture_energy.py)"""
    for name in NEW:
        assert not re.match(r"gpe_(set|bind)_", name)


def test_config_layout_is_unchanged():
    lib = capi.load()
    assert lib.gpe_sizeof_config() == C.sizeof(capi.gpe_config)
    assert [n for n, _ in capi.gpe_config._fields_][-3:] == ["mixture", "mix_g", "mix_norm"]
    assert re.search(r"int32_t\s+mixture;\s*float\s+mix_g\[3\];[^\n]*\n\s*float\s+mix_norm\[2\];[^\n]*\n\}\s*gpe_config;", _header())
    assert int(re.search(r"#define\s+GPE_ABI_VERSION\s+(\d+)", _header()).group(1)) == capi.GPE_ABI_VERSION == lib.gpe_abi_version()
    assert not any("energy" in n for n, _ in capi.gpe_config._fields_)
    assert lib.gpe_exchange_dbl_count() == 20                       # S_COUNT = 12 sums + 4 local + 4: the five new sums took free slots


def test_a_null_engine_is_refused():
    lib = capi.load()
    out = (C.c_double * 8)()
    assert lib.gpe_mixture_energy_weight(None, 1.0) == capi.GPE_ERR_INVALID
    assert lib.gpe_mixture_energy(None, out) == capi.GPE_ERR_INVALID


def test_w_riesz_stays_refused_for_a_mixture_at_create(monkeypatch):
    for k in [k for k in os.environ if k.startswith("GPE_") and k != "GPE_HIP_LIB"]:
        monkeypatch.delenv(k)
    lib = capi.load()
    c = gpe_pinn.GPEConfig(layers=[2, 64, 64, 2], mixture=True, mix_g=(1.0, 2.0, 0.5), mix_norm=(0.5, 0.5)).to_c()
    c.w_riesz = 1.0
    h = C.c_void_p()
    rc = lib.gpe_create(C.byref(c), 0, None, C.byref(h))
    assert rc == capi.GPE_ERR_INVALID and h.value is None and "w_riesz must be 0" in (lib.gpe_last_error(None) or b"").decode()


def test_the_python_surface_has_both_methods():
    assert callable(gpe_pinn.Engine.set_mixture_energy) and callable(gpe_pinn.Engine.mixture_energy)
    assert gpe_pinn.Engine.MIXTURE_ENERGY_FIELDS == ("E", "T1", "T2", "Q11", "Q22", "Q12", "den1", "den2")
