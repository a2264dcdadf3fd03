"""gpe_create refuses a bad configuration before it touches the device: every refusal of its first four phases (check_config,
describe_net, select_path), with the message the caller sees, and the order in which two broken rules are reported.  Raw gpe_config
structs through the C ABI: the library loads and refuses without a GPU.

Not reachable, so not here: "the Riesz energy term needs real psi ..." (two outputs already need complex psi with p = 3, which that
rule admits) and the 160 KB bound inside "fused path needs ..." (the deepest network the ABI admits, ten hidden layers of 64 in 3D,
still fits)."""
import ctypes as C
import os
import re

import pytest

import gpe_pinn
from gpe_pinn import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "gross-pitaevskii-eigenvalue-problem_amd", "csrc", "gpe_fused.h")) as _f:
    FWD_WAVES = int(re.search(r"#define\s+GPE_FWD_WAVES\s+(\d+)", _f.read()).group(1))

RES, FUSED, ENERGY = capi.NET_RESIDUAL, capi.PATH_FUSED, capi.LAMBDA_ENERGY
CPLX = dict(layers=[2, 64, 64, 2], complex_psi=1)           # a valid complex-psi network (p = 3 by default)

# id: (fields set on a valid [2,64,64,1] configuration ("layers" sets n_layers too), environment, substring of the message)
REFUSALS = {
    "abi": (dict(abi_version=capi.GPE_ABI_VERSION - 1), {}, "abi_version 1 != 2"),
    "too_few_layers": (dict(layers=[2, 1]), {}, "n_layers must be in [3,12]"),
    "too_many_layers": (dict(n_layers=capi.GPE_MAX_LAYERS + 1), {}, "n_layers must be in [3,12]"),
    "dim_0": (dict(layers=[0, 64, 64, 1]), {}, "dim must be 1..3"),
    "dim_4": (dict(layers=[4, 64, 64, 1]), {}, "dim must be 1..3"),
    "out_0": (dict(layers=[2, 64, 64, 0]), {}, "output width must be 1 or 2"),
    "out_3": (dict(layers=[2, 64, 64, 3]), {}, "output width must be 1 or 2"),
    "complex_one_output": (dict(complex_psi=1), {}, "complex psi needs out=2 and p=3"),
    "complex_p_2": (dict(CPLX, p=2), {}, "complex psi needs out=2 and p=3"),
    "real_two_outputs": (dict(layers=[2, 64, 64, 2]), {}, "real psi needs out=1"),
    "potential_5": (dict(potential=capi.POT_NONE + 1), {}, "Unknown potential type: 5"),
    "potential_negative": (dict(potential=-1), {}, "Unknown potential type: -1"),
    "hermite_base_2d": (dict(base_mode=0), {}, "Hermite base needs dim=1, out=1"),
    "p_0": (dict(p=0), {}, "power p must be in [1,32]"),
    "p_33": (dict(p=33), {}, "power p must be in [1,32]"),
    "rotation_real_psi": (dict(omega_rot=0.5), {}, "rotation needs complex psi and dim>=2"),
    "rotation_1d": (dict(layers=[1, 64, 64, 2], complex_psi=1, omega_rot=0.5), {}, "rotation needs complex psi and dim>=2"),
    "base_kind": (dict(base_kind=capi.BASE_PRECOMPUTED + 1), {}, "Unknown base kind: 3"),
    "envelope": (dict(envelope=capi.ENV_SIN + 1), {}, "Unknown envelope: 2"),
    "envelope_2d": (dict(envelope=capi.ENV_SIN), {}, "the boundary factor needs dim=1, out=1"),
    "riesz_kind": (dict(riesz_kind=capi.RIESZ_VARIATIONAL + 1), {}, "Unknown Riesz kind: 3"),
    "lambda_kind": (dict(lambda_kind=2), {}, "Unknown lambda kind: 2"),
    "energy_lambda_complex": (dict(CPLX, lambda_kind=ENERGY), {}, "the energy-functional lambda needs real psi (out=1) and an odd power p"),
    "energy_lambda_even_p": (dict(lambda_kind=ENERGY, p=2), {}, "the energy-functional lambda needs real psi (out=1) and an odd power p"),
    "reg_lam_rayleigh": (dict(w_reg_lam=1.0), {}, "the 1/lambda^2 regulariser needs the energy-functional lambda"),
    "reg_f_complex": (dict(CPLX, w_reg_f=1.0), {}, "the regularisers need real psi (out=1)"),
    "reg_f_eps_0": (dict(w_reg_f=1.0, reg_f_eps=0.0), {}, "regulariser eps must be > 0"),
    "reg_lam_eps_0": (dict(lambda_kind=ENERGY, w_reg_lam=1.0, reg_lam_eps=0.0), {}, "regulariser eps must be > 0"),
    "hidden_width_0": (dict(layers=[2, 64, 0, 1]), {}, "hidden width 0 out of range"),
    "hidden_width_1025": (dict(layers=[2, 1025, 64, 1]), {}, "hidden width 1025 out of range"),
    # describe_net
    "net_kind": (dict(net_kind=2), {}, "Unknown network kind: 2"),
    "residual_no_block": (dict(layers=[2, 64, 1], net_kind=RES), {}, "residual network: 1..4 blocks"),
    "residual_5_blocks": (dict(layers=[2] + [64] * 6 + [1], net_kind=RES), {}, "residual network: 1..4 blocks"),
    "residual_two_widths": (dict(layers=[2, 64, 32, 1], net_kind=RES), {}, "residual network: one hidden width"),
    # select_path
    "fused_one_hidden_layer": (dict(layers=[2, 64, 1], path=FUSED), {}, "fused path needs >=2 hidden layers of one width"),
    "fused_width_512": (dict(layers=[2, 512, 512, 1], path=FUSED), {}, "fused path needs >=2 hidden layers of one width"),
    "fused_residual_128": (dict(layers=[2, 128, 128, 1], net_kind=RES, path=FUSED), {}, "fused path needs >=2 hidden layers of one width"),
    "fused_residual_switched_off": (dict(layers=[2, 64, 64, 1], net_kind=RES, path=FUSED), {"GPE_RES_FUSED": "0"},
                                    "fused path needs >=2 hidden layers of one width"),
    "fwd_wg_per_cu_0": ({}, {"GPE_FWD_WG_PER_CU": "0"}, "GPE_FWD_WG_PER_CU=0: this build runs f_forward at 1..%d workgroups per CU" % FWD_WAVES),
    "fwd_wg_per_cu_beyond_the_build": ({}, {"GPE_FWD_WG_PER_CU": str(FWD_WAVES + 1)},
                                       "GPE_FWD_WG_PER_CU=%d: this build runs f_forward at 1..%d workgroups per CU" % (FWD_WAVES + 1, FWD_WAVES)),
}

# two rules broken at once: the earlier one's message is the one the caller sees.
# id: (fields, environment, the earlier rule's text, fields that break the later rule alone, the later rule's text)
ORDER = {
    "within_check_config": (dict(layers=[4, 64, 64, 1], potential=5), {}, "dim must be 1..3", dict(potential=5), "Unknown potential"),
    "check_config_before_describe_net": (dict(layers=[2, 64, 0, 1], net_kind=2), {}, "hidden width 0 out of range", dict(net_kind=2),
                                         "Unknown network kind"),
    "describe_net_before_select_path": (dict(layers=[2, 128, 64, 1], net_kind=RES, path=FUSED), {}, "residual network: one hidden width",
                                        dict(layers=[2, 128, 128, 1], net_kind=RES, path=FUSED), "fused path needs"),
    "configuration_before_switches": (dict(potential=5), {"GPE_FWD_WG_PER_CU": "0"}, "Unknown potential type: 5", {}, "GPE_FWD_WG_PER_CU"),
}


def config(**fields):
    c = gpe_pinn.GPEConfig(layers=fields.pop("layers", [2, 64, 64, 1])).to_c()
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def create(fields, env, monkeypatch):
    for k in [k for k in os.environ if k.startswith("GPE_") and k != "GPE_HIP_LIB"]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib = capi.load()
    c, h = config(**fields), C.c_void_p()
    rc = lib.gpe_create(C.byref(c), 0, None, C.byref(h))
    msg = (lib.gpe_last_error(None) or b"").decode()
    if rc == capi.GPE_OK:
        lib.gpe_destroy(h)
    return rc, msg, h.value


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal(name, monkeypatch):
    fields, env, text = REFUSALS[name]
    rc, msg, h = create(fields, env, monkeypatch)
    assert rc == capi.GPE_ERR_INVALID and h is None, (rc, msg)
    assert text in msg, msg


@pytest.mark.parametrize("name", sorted(ORDER))
def test_the_earlier_rule_is_the_one_reported(name, monkeypatch):
    fields, env, first, later_alone, second = ORDER[name]
    rc, msg, _ = create(fields, env, monkeypatch)
    assert rc == capi.GPE_ERR_INVALID and first in msg and second not in msg, (rc, msg)
    rc, msg, _ = create(later_alone, env, monkeypatch)          # (the later rule was really broken: alone, it refuses)
    assert rc == capi.GPE_ERR_INVALID and second in msg, (rc, msg)


VALID = {
    "fused": dict(layers=[2, 64, 64, 1]),
    "padded_to_128": dict(layers=[2, 100, 100, 100, 1]),
    "residual_fused": dict(layers=[1, 64, 64, 1], net_kind=RES),
    "generic": dict(layers=[2, 48, 1]),
    "wide": dict(layers=[3, 256, 256, 256, 1]),
}


@pytest.mark.parametrize("name", sorted(VALID))
def test_a_valid_configuration_fails_at_the_device_and_not_before(name, monkeypatch):
    """without a GPU the first HIP call of creation (hipSetDevice) is what fails: the configuration-only phases made none and passed"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rc, msg, h = create(VALID[name], {}, monkeypatch)
    assert rc == capi.GPE_ERR_HIP and h is None and msg.startswith("hipSetDevice:"), (rc, msg)
