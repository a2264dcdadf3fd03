"""gpe_create and a two-component mixture (gpe_config.mixture): every combination the engine refuses, with the message the caller sees and
the order in which two broken rules are reported -- raw gpe_config structs through the C ABI, no device (the pattern of
tests/test_create_refusals_cpu.py).  And the struct layout / ABI version the header and the ctypes binding agree on."""
import ctypes as C
import math
import os
import re

import pytest

import gpe_pinn
from gpe_pinn import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, ENERGY = capi.NET_RESIDUAL, capi.LAMBDA_ENERGY

# id: (fields set on a valid [2,64,64,2] mixture configuration, substring of the message), in the order check_config tests the rules
REFUSALS = [
    ("one_output", dict(layers=[2, 64, 64, 1]), "a mixture needs out=2 and p=3"),
    ("p_2", dict(p=2), "a mixture needs out=2 and p=3"),
    ("complex_psi", dict(complex_psi=1), "complex psi does not combine"),
    ("rotation", dict(omega_rot=0.5), "omega_rot must be 0"),
    ("base_mode", dict(base_mode=0), "base_mode must be -1"),
    ("envelope", dict(envelope=capi.ENV_SIN), "envelope must be GPE_ENV_NONE"),
    ("w_sym", dict(w_sym=1.0), "w_sym must be 0"),
    ("w_orth", dict(w_orth=1.0), "w_orth must be 0"),
    ("w_riesz", dict(w_riesz=1.0), "w_riesz must be 0"),
    ("lambda_kind", dict(lambda_kind=ENERGY), "lambda_kind must be GPE_LAMBDA_RAYLEIGH"),
    ("w_reg_f", dict(w_reg_f=1.0), "w_reg_f and w_reg_lam must be 0"),
    ("w_reg_lam", dict(w_reg_lam=1.0), "w_reg_f and w_reg_lam must be 0"),
    ("residual_blocks", dict(net_kind=RES), "residual blocks do not combine"),
    ("g11_nan", dict(mix_g=(math.nan, 1.0, 1.0)), "mix_g[0] is not finite"),
    ("g12_inf", dict(mix_g=(1.0, 1.0, math.inf)), "mix_g[2] is not finite"),
    ("n1_zero", dict(mix_norm=(0.0, 1.0)), "mix_norm[0] must be finite and > 0"),
    ("n2_negative", dict(mix_norm=(1.0, -0.5)), "mix_norm[1] must be finite and > 0"),
    ("n2_nan", dict(mix_norm=(1.0, math.nan)), "mix_norm[1] must be finite and > 0"),
]
BY_ID = {r[0]: r for r in REFUSALS}
# consecutive rules of the list above that can be broken together (a different message each): the earlier one is reported
ORDER = [(a, b) for a, b in zip(REFUSALS[:-1], REFUSALS[1:]) if a[2] != b[2] and not (set(a[1]) & set(b[1]))]


def config(**fields):
    c = gpe_pinn.GPEConfig(layers=fields.pop("layers", [2, 64, 64, 2]), mixture=True, mix_g=(1.0, 2.0, 0.5), mix_norm=(0.5, 0.5)).to_c()
    for k, v in fields.items():
        if isinstance(v, tuple):
            for i, vi in enumerate(v):
                getattr(c, k)[i] = vi
        else:
            setattr(c, k, v)
    return c


def create(fields, monkeypatch):
    for k in [k for k in os.environ if k.startswith("GPE_") and k != "GPE_HIP_LIB"]:
        monkeypatch.delenv(k)
    lib = capi.load()
    c, h = config(**fields), C.c_void_p()
    rc = lib.gpe_create(C.byref(c), 0, None, C.byref(h))
    msg = (lib.gpe_last_error(None) or b"").decode()
    if rc == capi.GPE_OK:
        lib.gpe_destroy(h)
    return rc, msg, h.value


@pytest.mark.parametrize("name", [r[0] for r in REFUSALS])
def test_refusal(name, monkeypatch):
    _, fields, text = BY_ID[name]
    rc, msg, h = create(dict(fields), monkeypatch)
    assert rc == capi.GPE_ERR_INVALID and h is None, (rc, msg)
    assert text in msg, msg


@pytest.mark.parametrize("first,second", ORDER, ids=[f"{a[0]}-before-{b[0]}" for a, b in ORDER])
def test_the_earlier_rule_is_the_one_reported(first, second, monkeypatch):
    rc, msg, _ = create(dict(first[1], **second[1]), monkeypatch)
    assert rc == capi.GPE_ERR_INVALID and first[2] in msg and second[2] not in msg, (rc, msg)


def test_a_mixture_rule_comes_before_the_rules_of_the_other_problems(monkeypatch):
    """base_mode >= 0 with two outputs also breaks "Hermite base needs dim=1, out=1"; rotation also breaks "rotation needs complex psi":
    the caller of a mixture is told about the mixture"""
    rc, msg, _ = create(dict(base_mode=0), monkeypatch)
    assert rc == capi.GPE_ERR_INVALID and "a mixture has no analytic base" in msg and "Hermite" not in msg, msg
    rc, msg, _ = create(dict(omega_rot=0.3), monkeypatch)
    assert rc == capi.GPE_ERR_INVALID and "a mixture has no rotating frame" in msg and "needs complex psi" not in msg, msg


def test_two_real_outputs_without_the_flag_stay_refused(monkeypatch):
    rc, msg, _ = create(dict(mixture=0), monkeypatch)
    assert rc == capi.GPE_ERR_INVALID and "real psi needs out=1" in msg, msg


@pytest.mark.parametrize("layers", [[2, 64, 64, 2], [2, 72, 72, 72, 2], [3, 256, 256, 2], [1, 48, 2]])
def test_a_valid_mixture_fails_at_the_device_and_not_before(layers, monkeypatch):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rc, msg, h = create(dict(layers=layers), monkeypatch)
    assert rc == capi.GPE_ERR_HIP and h is None and msg.startswith("hipSetDevice:"), (rc, msg)


def test_struct_layout_and_abi_version_agree_with_the_header():
    lib = capi.load()
    assert lib.gpe_sizeof_config() == C.sizeof(capi.gpe_config)
    hdr = open(os.path.join(ROOT, "include", "gpe_hip.h")).read()
    assert int(re.search(r"#define\s+GPE_ABI_VERSION\s+(\d+)", hdr).group(1)) == capi.GPE_ABI_VERSION == lib.gpe_abi_version()
    # the new fields are the last of the struct, in the header's order, and the new entry points are bound
    assert [n for n, _ in capi.gpe_config._fields_][-3:] == ["mixture", "mix_g", "mix_norm"]
    assert re.search(r"int32_t\s+mixture;\s*float\s+mix_g\[3\];[^\n]*\n\s*float\s+mix_norm\[2\];[^\n]*\n\}\s*gpe_config;", hdr)
    assert capi.gpe_config.mix_norm.offset + 8 == C.sizeof(capi.gpe_config) or C.sizeof(capi.gpe_config) % 8 == 0
    for name in ("gpe_set_mixture", "gpe_mixture_scalars"):
        assert name in capi.SYMBOLS and hasattr(lib, name)


def test_config_roundtrip_of_the_mixture_fields():
    c = gpe_pinn.GPEConfig(layers=[2, 64, 64, 2], mixture=True, mix_g=(1.5, 0.25, -0.5), mix_norm=(0.75, 0.25)).to_c()
    assert c.mixture == 1 and list(c.mix_g) == [1.5, 0.25, -0.5] and list(c.mix_norm) == [0.75, 0.25]
    assert gpe_pinn.GPEConfig(layers=[2, 64, 64, 1]).to_c().mixture == 0
