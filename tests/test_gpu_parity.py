"""Parity tests proper: the HIP engine (through the C ABI) against the CPU oracle and against the golden vectors
produced by the imported reference.  Run on the GPU box:  python -m pytest tests -m gpu -x -q

Tolerances (fp32 kernels vs fp64 oracle unless noted):
  NN output jets            rel 1e-5 of the channel maximum
  mu (Rayleigh quotient)    rel 2e-5          loss pieces   rel 1e-4 (differences of O(1) terms)
  gradient                  rel 5e-5 of max|g| vs the oracle ; rel 5e-4 vs the reference's fp32 autograd gradient
  trajectories              as in tests/test_oracle_golden.py (fp32 chaos grows with the step count)
"""
import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import GPEConfig, Engine
from oracle import gpe_oracle as go
from tests import helpers as H

pytestmark = pytest.mark.gpu

PATHS = {"generic": gpe_pinn.PATH_GENERIC, "fused": gpe_pinn.PATH_FUSED}


def cfg_from_problem(pb: go.Problem, **kw) -> GPEConfig:
    d = dict(layers=list(pb.layers), activation=pb.activation, complex_psi=pb.complex_psi, kinetic_coeff=pb.kinetic_coeff,
             potential=pb.potential, pot_scale=pb.pot_scale, omega=tuple(pb.omega), pot_a=pb.pot_a, pot_v0=pb.pot_v0,
             pot_k=pb.pot_k, omega_rot=pb.omega_rot, gamma=pb.gamma, p=pb.p, abs_power=pb.abs_power,
             base_mode=pb.base_mode, base_deriv=pb.base_deriv, perturb_scale=pb.perturb_scale,
             bc_nn_scale=pb.bc_nn_scale, w_pde=pb.w_pde, w_bc=pb.w_bc, w_norm=pb.w_norm, w_sym=pb.w_sym,
             w_orth=pb.w_orth, sym_sign=pb.sym_sign, dx=pb.dx, n_global=pb.n_global, base_kind=pb.base_kind,
             envelope=pb.envelope, box_L=pb.box_L, env_L=pb.env_L, w_riesz=pb.w_riesz, riesz_kind=pb.riesz_kind, net_kind=pb.net_kind,
             lambda_kind=pb.lambda_kind, w_reg_f=pb.w_reg_f, reg_f_eps=pb.reg_f_eps, w_reg_lam=pb.w_reg_lam, reg_lam_eps=pb.reg_lam_eps)
    d.update(kw)
    return GPEConfig(**d)


def make_engine(pb, flat, x, x_bc=None, **kw):
    cfg = cfg_from_problem(pb, **kw)
    if x_bc is None:
        cfg.w_bc = 0.0
    eng = Engine(cfg)
    eng.set_params(flat)
    eng.bind_points(torch.as_tensor(np.asarray(x, np.float32), device="cuda"))
    if x_bc is not None:
        eng.bind_boundary(torch.as_tensor(np.asarray(x_bc, np.float32), device="cuda"))
    return eng


CASES = {
    # name: (Problem kwargs, N, fused-capable)
    "1d_64x3_refine": (dict(layers=[1, 64, 64, 64, 1], activation=1, kinetic_coeff=1.0, pot_scale=1.0, gamma=5.0, p=3,
                            base_mode=0, perturb_scale=0.05, dx=12 / 499), 500, True),
    "1d_32x4_nb_sym": (dict(layers=[1, 32, 32, 32, 32, 1], gamma=1.0, p=3, base_mode=0, base_deriv=1, w_sym=5.0,
                            dx=12 / 299), 300, True),
    "1d_64x4_m3_p4_odd": (dict(layers=[1, 64, 64, 64, 64, 1], activation=1, gamma=2.0, p=4, base_mode=3, perturb_scale=0.1,
                               w_sym=5.0, sym_sign=-1.0, dx=12 / 1000), 1001, True),
    "1d_abs_power_p2": (dict(layers=[1, 32, 32, 1], gamma=3.0, p=2, abs_power=True, base_mode=1, dx=0.03), 333, True),
    # beta-scaled SHIFTED trap V = beta/2 omega^2 (x - center)^2 (refine/vary_potential_parameter_harmonic.py:231-240): beta = 0.7, omega = 3
    "1d_shifted_beta_trap": (dict(layers=[1, 32, 32, 32, 1], activation=1, kinetic_coeff=1.0, pot_scale=0.35, omega=(3.0, 1.0, 1.0),
                                  pot_a=0.7, gamma=4.0, dx=0.03), 300, True),
    "1d_gaussian_pot": (dict(layers=[1, 32, 32, 32, 1], potential=go.POT_GAUSSIAN, pot_a=0.5, gamma=1.0, dx=0.03), 200, True),
    "1d_periodic_pot": (dict(layers=[1, 32, 32, 32, 1], potential=go.POT_PERIODIC, gamma=1.0, dx=0.03), 200, True),
    "2d_64x4_g500": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=500.0, dx=36 / 777), 777, True),
    "2d_32x3": (dict(layers=[2, 32, 32, 32, 1], gamma=10.0, dx=0.05), 100, True),
    "3d_64x3_aniso": (dict(layers=[3, 64, 64, 64, 1], gamma=20.0, dx=0.01, omega=(1.0, 1.4, 2.0)), 130, True),
    "2d_64x3_complex_rot": (dict(layers=[2, 64, 64, 64, 2], complex_psi=True, gamma=30.0, dx=0.02, omega_rot=0.8), 200, True),
    "2d_N1": (dict(layers=[2, 64, 64, 1], gamma=3.0, dx=0.1), 1, True),
    "2d_N17_ragged": (dict(layers=[2, 64, 64, 1], gamma=3.0, dx=0.1), 17, True),
    "2d_128x3_cfg3like": (dict(layers=[2, 128, 128, 128, 1], gamma=100.0, dx=0.01), 300, True),
    "2d_128x5_cfg3": (dict(layers=[2, 128, 128, 128, 128, 128, 1], gamma=500.0, dx=0.01), 200, True),
    "2d_128x6_complex_cfg4like": (dict(layers=[2, 128, 128, 2], complex_psi=True, gamma=50.0, omega_rot=0.8, dx=0.01), 150, True),
    "2d_128x6_complex_cfg4": (dict(layers=[2, 128, 128, 128, 128, 128, 128, 2], complex_psi=True, gamma=50.0, omega_rot=0.8,
                                   dx=0.01), 150, True),
    "1d_128x2": (dict(layers=[1, 128, 128, 1], gamma=5.0, base_mode=0, dx=0.02), 130, True),
    "3d_256x2_cfg5like": (dict(layers=[3, 256, 256, 1], gamma=100.0, dx=0.01, omega=(1.0, 1.4, 2.0)), 64, False),
    # BASELINE configs[4] at its true shape: 6 hidden layers of 256, 3D anisotropic trap, g = 1000.  N = 300 / 4099 make the
    # split-K weight-gradient kernel of the generic set run 2 / 17 chunks of 256 points with a ragged last chunk and tile.
    "3d_256x6_cfg5_N300": (dict(layers=[3, 256, 256, 256, 256, 256, 256, 1], gamma=1000.0, dx=0.004, omega=(1.0, 1.4, 2.0)), 300, True),
    "3d_256x6_cfg5_N4099": (dict(layers=[3, 256, 256, 256, 256, 256, 256, 1], gamma=1000.0, dx=0.0003, omega=(1.0, 1.4, 2.0)), 4099, True),
    "3d_128x6_N300": (dict(layers=[3, 128, 128, 128, 128, 128, 128, 1], gamma=1000.0, dx=0.004, omega=(1.0, 1.4, 2.0)), 300, True),
    "3d_128x3_N1000": (dict(layers=[3, 128, 128, 128, 1], gamma=100.0, dx=0.001, omega=(1.0, 1.4, 2.0)), 1000, True),
    "2d_256x3": (dict(layers=[2, 256, 256, 256, 1], gamma=100.0, dx=0.01), 333, True),
    "1d_256x2": (dict(layers=[1, 256, 256, 1], gamma=5.0, base_mode=0, dx=0.02), 130, True),
    # BASELINE configs[0], literally: 1D harmonic trap, g = 0 (linear Schroedinger), 4 x 32 tanh MLP, 2048 points on [-10, 10]
    "1d_32x4_cfg1_g0_N2048": (dict(layers=[1, 32, 32, 32, 32, 1], gamma=0.0, dx=20.0 / 2047), 2048, True),
    # Riesz energy in d > 1 (row f4): the reference's 2D point-sum form and the variational quotient used by the accuracy runs
    "2d_riesz_sum": (dict(layers=[2, 64, 64, 64, 1], gamma=100.0, kinetic_coeff=1.0, pot_scale=1.0, w_riesz=0.05, riesz_kind=go.RIESZ_SUM,
                          dx=36 / 400), 400, True),
    "2d_riesz_variational": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=500.0, w_riesz=2.0, riesz_kind=go.RIESZ_VARIATIONAL, dx=36 / 900),
                             900, True),
    # complex psi in the rotating frame with the variational energy E[psi / |psi|] - Omega <L_z> (what keeps cfg4 on the vortex-lattice
    # state; no reference code: oracle = definition, cross-checked against fp64 autograd in tests/test_oracle_autograd.py)
    "2d_complex_rot_variational": (dict(layers=[2, 64, 64, 64, 2], complex_psi=True, gamma=30.0, omega_rot=0.8, w_riesz=1.5,
                                        riesz_kind=go.RIESZ_VARIATIONAL, dx=36 / 600), 600, True),
    "2d_128x6_complex_rot_variational_cfg4": (dict(layers=[2, 128, 128, 128, 128, 128, 128, 2], complex_psi=True, gamma=500.0, omega_rot=0.8,
                                                   w_riesz=1.0, riesz_kind=go.RIESZ_VARIATIONAL, dx=36 / 400), 400, True),
    "3d_riesz_variational": (dict(layers=[3, 128, 128, 128, 1], gamma=100.0, omega=(1.0, 1.4, 2.0), w_riesz=1.0,
                                  riesz_kind=go.RIESZ_VARIATIONAL, dx=0.01), 500, True),
    # the 2D classes' loss (src/gross_pitaevskii_2D.py:154-242): energy-functional lambda (its gradient branch is carried through the reverse
    # pass), 1/(mean u^2 + eps) and 1/(lambda^2 + eps) regularisers, with and without the unnormalised Riesz sum (which dwarfs the rest at g = 500)
    "2d_class_loss_64x4": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=500.0, kinetic_coeff=1.0, pot_scale=1.0, w_norm=0.0, w_riesz=1.0,
                                riesz_kind=go.RIESZ_SUM, lambda_kind=go.LAMBDA_ENERGY, w_reg_f=1.0, w_reg_lam=1.0, abs_power=True, dx=1.0), 777, True),
    "2d_energy_lambda_regs_64x4": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=100.0, kinetic_coeff=1.0, pot_scale=1.0, w_norm=0.0,
                                        lambda_kind=go.LAMBDA_ENERGY, w_reg_f=1.0, w_reg_lam=1.0, dx=1.0), 500, True),
    "2d_energy_lambda_128x3": (dict(layers=[2, 128, 128, 128, 1], gamma=100.0, lambda_kind=go.LAMBDA_ENERGY, w_reg_lam=0.5, reg_lam_eps=1e-3,
                                    dx=0.01), 300, True),
    "3d_energy_lambda_p5_256x2": (dict(layers=[3, 256, 256, 1], gamma=3.0, p=5, omega=(1.0, 1.4, 2.0), lambda_kind=go.LAMBDA_ENERGY,
                                       w_riesz=0.5, riesz_kind=go.RIESZ_VARIATIONAL, dx=0.01), 130, True),
    "1d_reg_f_rayleigh": (dict(layers=[1, 32, 32, 32, 1], gamma=2.0, base_mode=0, w_reg_f=0.5, reg_f_eps=0.05, dx=12 / 299), 300, True),
    "2d_energy_lambda_N1": (dict(layers=[2, 64, 64, 1], gamma=3.0, kinetic_coeff=1.0, pot_scale=1.0, w_norm=0.0, lambda_kind=go.LAMBDA_ENERGY,
                                 w_reg_f=1.0, w_reg_lam=1.0, dx=1.0), 1, True),
    # residual-block networks (refine/box_to_gaussian_pinn_simulation.py:52-63,100-130): generic set
    "1d_residual_64x2blocks": (dict(layers=[1, 64, 64, 64, 1], net_kind=go.NET_RESIDUAL, activation=1, kinetic_coeff=1.0,
                                    potential=go.POT_GAUSSIAN, pot_a=0.5, gamma=3.0, p=4, base_mode=1, perturb_scale=0.05, dx=0.03), 333, True),
    # (round 4: one or two residual blocks of width 32 / 64 run on the cooperative whole-network kernels, <..., RES>)
    "1d_residual_64x1block": (dict(layers=[1, 64, 64, 1], net_kind=go.NET_RESIDUAL, activation=1, kinetic_coeff=1.0, gamma=2.0, base_mode=0,
                                   perturb_scale=0.05, dx=0.03), 200, True),
    "2d_residual_64x2blocks": (dict(layers=[2, 64, 64, 64, 1], net_kind=go.NET_RESIDUAL, gamma=20.0, dx=0.01), 300, True),
    "3d_residual_32x2blocks": (dict(layers=[3, 32, 32, 32, 1], net_kind=go.NET_RESIDUAL, gamma=5.0, omega=(1.0, 1.4, 2.0), dx=0.01), 130, True),
    "2d_residual_128x3blocks": (dict(layers=[2, 128, 128, 128, 128, 1], net_kind=go.NET_RESIDUAL, gamma=20.0, dx=0.01), 300, False),
    # four and five hidden -> hidden maps at H <= 64 (round 4: on the cooperative whole-network kernels; the per-wave-tile kernels hold three)
    "2d_64x5_four_maps": (dict(layers=[2, 64, 64, 64, 64, 64, 1], gamma=100.0, dx=0.01), 777, True),
    "1d_64x6_five_maps": (dict(layers=[1, 64, 64, 64, 64, 64, 64, 1], gamma=5.0, base_mode=1, dx=12 / 499), 500, True),
    "1d_shifted_tanh_64x5_four_maps": (dict(layers=[1, 64, 64, 64, 64, 64, 1], activation=1, kinetic_coeff=1.0, pot_scale=1.0, gamma=5.0, base_mode=0,
                                            perturb_scale=0.05, dx=12 / 299), 300, True),
    "3d_64x5_four_maps": (dict(layers=[3, 64, 64, 64, 64, 64, 1], gamma=20.0, omega=(1.0, 1.4, 2.0), dx=0.01), 300, True),
    "2d_32x6_five_maps_sym": (dict(layers=[2, 32, 32, 32, 32, 32, 32, 1], gamma=10.0, dx=0.01), 401, True),
    "2d_48x5_pads_to_64_four_maps": (dict(layers=[2, 48, 48, 48, 48, 48, 1], gamma=10.0, dx=0.01), 300, True),
    # hidden widths without an MFMA kernel instance: the fused path runs them zero-padded to the next instantiated width (plain tanh only);
    # the generic set takes them as given
    "2d_100x2_odd_width": (dict(layers=[2, 100, 100, 1], gamma=1.0, dx=0.01), 77, True),
    "2d_100x3_reference_2d_arch": (dict(layers=[2, 100, 100, 100, 1], gamma=100.0, kinetic_coeff=1.0, pot_scale=1.0, dx=0.01), 500, True),
    "2d_ragged_48_64_32": (dict(layers=[2, 48, 64, 32, 1], gamma=10.0, dx=0.01), 300, True),
    "3d_200x2_pads_to_256": (dict(layers=[3, 200, 200, 1], gamma=20.0, omega=(1.0, 1.4, 2.0), dx=0.01), 130, True),
    "1d_20x3_pads_to_32": (dict(layers=[1, 20, 20, 20, 1], gamma=2.0, base_mode=1, dx=0.03), 333, True),
    "1d_shifted_tanh_48x3_pads_to_64": (dict(layers=[1, 48, 48, 48, 1], activation=1, kinetic_coeff=1.0, pot_scale=1.0, gamma=5.0, base_mode=2,
                                             perturb_scale=0.05, dx=12 / 499), 500, True),
    "2d_shifted_tanh_100x3_pads_to_128": (dict(layers=[2, 100, 100, 100, 1], activation=1, gamma=50.0, dx=0.01), 300, True),
    "2d_complex_72x3_pads_to_128": (dict(layers=[2, 72, 72, 72, 2], complex_psi=True, gamma=30.0, omega_rot=0.8, dx=0.02), 200, True),
    "1d_single_hidden": (dict(layers=[1, 64, 1], gamma=1.0, dx=0.01, base_mode=1), 50, False),
    # the symmetry batch (x -> [x ; -x], value only: the (1, 0) instances of the reverse kernels, as the pre-training step runs them) beyond
    # 1D plain MLPs at H <= 64: five maps in 2D, H = 128, residual blocks
    "2d_32x6_five_maps_w_sym": (dict(layers=[2, 32, 32, 32, 32, 32, 32, 1], gamma=10.0, dx=0.01, w_sym=5.0), 401, True),
    "2d_128x3_w_sym": (dict(layers=[2, 128, 128, 128, 1], gamma=100.0, dx=0.01, w_sym=5.0), 300, True),
    "1d_residual_64x2blocks_w_sym": (dict(layers=[1, 64, 64, 64, 1], net_kind=go.NET_RESIDUAL, activation=1, kinetic_coeff=1.0,
                                          potential=go.POT_GAUSSIAN, pot_a=0.5, gamma=3.0, p=4, base_mode=1, perturb_scale=0.05, w_sym=5.0,
                                          sym_sign=-1.0, dx=0.03), 333, True),
}


def close(a, b, rtol, atol):
    """max|a-b| <= rtol*max|b| + atol  (atol covers N=1 cases where the single value is a cancelling sum of O(1) terms)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max()) <= rtol * float(np.abs(b).max()) + atol


def _inputs(kw, N, seed=0, scale=0.3):
    rng = np.random.default_rng(seed)
    layers = kw["layers"]
    d = layers[0]
    x = np.linspace(-6, 6, N).reshape(-1, 1) if d == 1 else rng.uniform(-3, 3, (N, d))
    x = x.astype(np.float32)
    flat = (rng.normal(0, 1, go.param_count(layers, kw.get("net_kind", 0))) * scale).astype(np.float32)
    x_bc = (np.array([[-6.0], [6.0]]) if d == 1 else rng.uniform(-3, 3, (5, d))).astype(np.float32)
    return x, flat, x_bc


def _scale(kw):
    """weight scale ~ 2.4 / sqrt(H): keeps tanh out of saturation through deep wide nets, so every jet channel stays O(1)"""
    w = max(kw["layers"][1:-1])
    return 0.3 if w <= 64 else (0.15 if w <= 128 else 0.1)


# shapes whose whole-network (fused) kernel is not built yet: they run on the generic layer-wise set only
PENDING_FUSED = set()


def _case_params():
    out = []
    for name, (kw, N, fused_ok) in CASES.items():
        out.append(pytest.param(name, "generic", id=f"{name}-generic"))
        if fused_ok:
            out.append(pytest.param(name, "fused", id=f"{name}-fused"))
    return out


@pytest.mark.parametrize("name,path", _case_params())
def test_step_matches_oracle(name, path):
    kw, N, _ = CASES[name]
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    if path == "fused" and name in PENDING_FUSED:
        pytest.skip("no fused kernel for this shape yet (generic set covers it)")
    osc, ograd, ores = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64))
    _, oskip, oplain = go.expand_layers(pb.layers, pb.net_kind)
    ojets, _ = go.mlp_forward(go.unflatten(flat.astype(np.float64), pb.layers, pb.net_kind), x.astype(np.float64), pb.activation,
                              skip=oskip, plain_tanh=oplain)
    eng = make_engine(pb, flat, x, x_bc, path=PATHS[path])
    assert eng.active_path == PATHS[path]
    jets = eng.forward_jets(torch.as_tensor(x, device="cuda")).cpu().numpy()
    for c in range(jets.shape[0]):
        assert close(jets[c], ojets[c], 1e-5, 2e-6), f"jet channel {c}"
    val = eng.forward(torch.as_tensor(x, device="cuda")).cpu().numpy()
    assert close(val, ojets[0], 1e-5, 2e-6)
    rs, psi, res = eng.residual()
    assert close(psi.cpu().numpy(), ores["psi"], 5e-6, 2e-6)
    assert close(res.cpu().numpy(), ores["residual"], 2e-5, 1e-5)
    sc = eng.step()
    # a single point makes mu = u*Hu/u^2 a quotient of two cancelling O(1e-2) sums: fp32 round-off is 10x larger there
    f = 10.0 if N < 4 else 1.0
    for k, tol in (("mu", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("bc", 1e-4), ("norm", 2e-4), ("sym", 1e-4), ("riesz", 1e-4), ("reg", 1e-4)):
        assert abs(sc[k] - osc[k]) <= f * tol * max(abs(osc[k]), 1e-6), (k, sc[k], osc[k])
    assert abs(rs["loss"] - osc["loss"]) <= f * 1e-4 * abs(osc["loss"])
    grad = eng.get_grad()
    assert H.rel_err(grad, ograd) < f * 5e-5
    assert not H.block_failures(grad, ograd, pb.layers, pb.net_kind, f)         # ... and per weight matrix / bias, of the block's own maximum
    assert abs(sc["grad_norm"] - np.linalg.norm(ograd)) < f * 1e-4 * np.linalg.norm(ograd)
    # Adam + clip on the device vs the oracle's optimiser (first step moves every weight by ~lr)
    new, _, _ = go.optimizer_step(go.OptState(lr0=1e-3), flat, ograd, osc["loss"])
    d = np.abs(eng.get_params() - new)
    assert np.quantile(d, 0.99) < 2e-5 and d.max() < 2.1e-3
    eng.close()


def test_fused_and_generic_agree_full_size():
    """BASELINE north-star size (1 048 576 points, [2,64x4,1]): the two kernel sets are independent implementations;
    their sums and gradients must agree at full size (size-independent cross-check, no oracle needed)."""
    N = 1 << 20
    kw = dict(layers=[2, 64, 64, 64, 64, 1], gamma=500.0, dx=(16.0 / 1023) ** 2)
    rng = np.random.default_rng(1)
    xs = np.linspace(-8, 8, 1024, dtype=np.float32)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    x = np.stack([X.ravel(), Y.ravel()], 1)
    flat = (rng.normal(0, 1, go.param_count(kw["layers"])) * 0.2).astype(np.float32)
    pb = go.Problem(**kw)
    outs = {}
    for path in ("generic", "fused"):
        eng = make_engine(pb, flat, x, None, path=PATHS[path])
        sc = eng.step()
        outs[path] = (sc, eng.get_grad())
        eng.close()
    (a, ga), (b, gb) = outs["generic"], outs["fused"]
    assert abs(a["mu"] - b["mu"]) < 1e-5 * abs(a["mu"])
    assert abs(a["loss"] - b["loss"]) < 1e-4 * abs(a["loss"])
    assert H.rel_err(gb, ga) < 2e-4


def test_deep_h64_network_on_the_cooperative_kernels_at_a_large_batch():
    """[2,64x5,1] (four hidden -> hidden maps) at 300 001 points: cooperative whole-network kernels at a size where three-map networks take
    the per-wave-tile kernels -- against the generic set (independent implementation) and the fp64 oracle."""
    kw = dict(layers=[2, 64, 64, 64, 64, 64, 1], gamma=50.0, dx=0.01)
    N = 300001
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    a = make_engine(pb, flat, x, x_bc)
    k = a.active_kernels
    assert a.active_path == gpe_pinn.PATH_FUSED and k["fwd"].startswith("f_forward_coop<64") and k["bwd"].startswith("f_backward_coop<64"), k
    sa = a.step(); ga = a.get_grad(); a.close()
    b = make_engine(pb, flat, x, x_bc, path=gpe_pinn.PATH_GENERIC)
    sb = b.step(); gb = b.get_grad(); b.close()
    assert abs(sa["loss"] - sb["loss"]) <= 1e-4 * abs(sb["loss"]) and abs(sa["mu"] - sb["mu"]) <= 2e-5 * abs(sb["mu"])
    assert H.rel_err(ga, gb) < 2e-4
    osc, ograd = go.sharded_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64), chunk=65536, threads=8)
    assert abs(sa["loss"] - osc["loss"]) <= 1e-4 * abs(osc["loss"]) and abs(sa["mu"] - osc["mu"]) <= 2e-5 * abs(osc["mu"])
    assert H.rel_err(ga, ograd) < 5e-5


@pytest.mark.parametrize("extra", [{}, dict(kinetic_coeff=1.0, pot_scale=1.0, w_norm=0.0, w_riesz=0.05, riesz_kind=go.RIESZ_SUM,
                                            lambda_kind=go.LAMBDA_ENERGY, w_reg_f=1.0, w_reg_lam=1.0)], ids=["north_star_loss", "2d_class_loss"])
def test_shard_additivity_two_engines_one_gpu(extra):
    """world_size = 2 emulated on one GPU: two engines own the two halves of the points, the exchange buffers are
    summed by hand (what the RCCL all-reduce does), and the result must equal the single-engine step.  Second case: the 2D classes' loss,
    whose lambda branch is built from the exchanged energy sums."""
    kw = dict(layers=[2, 64, 64, 64, 1], gamma=50.0, dx=0.01, **extra)
    N = 4099
    x, flat, x_bc = _inputs(kw, N)
    pb = go.Problem(**kw, n_global=N)
    full = make_engine(pb, flat, x, x_bc)
    ref = full.step()
    gref = full.get_grad()
    pref = full.get_params()
    lo = N // 2
    engs = [make_engine(pb, flat, x[:lo], x_bc, world_size=2), make_engine(pb, flat, x[lo:], x_bc, world_size=2)]
    for e in engs:
        e.step_begin()
    tot = engs[0].exchange_sums + engs[1].exchange_sums
    for e in engs:
        e.exchange_sums.copy_(tot)
        e.step_backward()
    gt = engs[0].exchange_grad + engs[1].exchange_grad
    for e in engs:
        e.exchange_grad.copy_(gt)
        e.step_update()
    scs = [e.read_scalars() for e in engs]
    for sc in scs:
        assert abs(sc["mu"] - ref["mu"]) < 1e-6 * abs(ref["mu"])
        assert abs(sc["loss"] - ref["loss"]) < 1e-5 * abs(ref["loss"])
        assert abs(sc["bc"] - ref["bc"]) < 1e-6 * abs(ref["bc"])
    assert H.rel_err(engs[0].get_grad(), gref) < 1e-5
    np.testing.assert_array_equal(engs[0].get_params(), engs[1].get_params())     # replicas stay bit-identical
    assert np.abs(engs[0].get_params() - pref).max() < 2e-5


@pytest.mark.parametrize("name", H.refine_names())
@pytest.mark.parametrize("path", ["generic", "fused"])
def test_golden_refine_oplevel(name, path):
    """Engine vs numbers produced by the reference's own refine/ classes (tests/golden/make_golden.py)."""
    fx = H.load_fx(name)
    pb = H.problem_from_refine(fx)
    eng = make_engine(pb, fx["flat0"], fx["x"], H.bc_points(fx), path=PATHS[path])
    xt = torch.as_tensor(fx["x"], device="cuda")
    assert H.rel_err(eng.forward(xt).cpu().numpy(), fx["nn_out"]) < 1e-5
    rs, psi, res = eng.residual()
    assert H.rel_err(psi.cpu().numpy(), fx["u"]) < 2e-6
    assert abs(rs["mu"] - float(fx["lam"])) < 2e-5 * max(1.0, abs(float(fx["lam"])))
    assert H.rel_err(res.cpu().numpy(), fx["residual"]) < 1e-4
    sc = eng.step()
    assert abs(sc["pde"] - float(fx["pde_loss"])) < 2e-4 * max(1e-3, float(fx["pde_loss"]))
    assert abs(sc["bc"] - float(fx["bc_loss"])) < 1e-5 * max(1e-6, float(fx["bc_loss"])) + 1e-12
    assert abs(sc["norm"] - float(fx["norm_loss"])) < 1e-4 * max(1e-3, float(fx["norm_loss"]))
    assert abs(sc["loss"] - float(fx["total"])) < 1e-4 * max(1e-3, float(fx["total"]))
    assert H.rel_err(eng.get_grad(), fx["grad0"]) < 5e-4
    eng.close()


@pytest.mark.parametrize("name", H.nb_names())
@pytest.mark.parametrize("path", ["generic", "fused"])
def test_golden_notebook_oplevel(name, path):
    fx = H.load_fx(name)
    pb = H.problem_from_nb(fx)
    eng = make_engine(pb, fx["flat0"], fx["x"], H.bc_points(fx), path=PATHS[path])
    rs, psi, res = eng.residual()
    assert H.rel_err(psi.cpu().numpy(), fx["u"]) < 2e-6
    assert abs(rs["mu"] - float(fx["lam"])) < 5e-5 * max(1.0, abs(float(fx["lam"])))
    assert H.rel_err(res.cpu().numpy(), fx["residual"]) < 2e-4
    sc = eng.step()
    assert abs(sc["sym"] - float(fx["sym_loss"])) < 1e-4 * max(1e-6, float(fx["sym_loss"]))
    assert abs(sc["loss"] - float(fx["total"])) < 2e-4 * float(fx["total"])
    assert H.rel_err(eng.get_grad(), fx["grad0"]) < 5e-4
    eng.close()


@pytest.mark.parametrize("name", ["fx_refine_m0_g0_64x3.npz", "fx_refine_m0_g50_64x3.npz", "fx_refine_m2_g10_32x4.npz"])
def test_golden_refine_trace(name):
    """(loss, mu, lr) over 25 epochs of the reference loop (Adam, clip 1.0, cosine scheduler stepped with the loss)."""
    fx = H.load_fx(name)
    pb = H.problem_from_refine(fx)
    eng = make_engine(pb, fx["flat0"], fx["x"], H.bc_points(fx), lr=1e-3, sched=gpe_pinn.SCHED_COSINE_LOSS)
    n = 25
    eng.run(n)                                          # enqueued back to back, scheduler on the device
    hist = eng.read_history(1, n)
    loss = np.array([h["loss"] for h in hist]); mu = np.array([h["mu"] for h in hist])
    lr = np.array([h["lr"] for h in hist]); gn = np.array([h["grad_norm"] for h in hist])
    assert [int(h["step"]) for h in hist] == list(range(1, n + 1))
    np.testing.assert_allclose(lr, fx["trace_lr"][:n], rtol=2e-3, atol=1e-9)
    np.testing.assert_allclose(loss[:10], fx["trace_loss"][:10], rtol=2e-3)
    np.testing.assert_allclose(mu[:10], fx["trace_mu"][:10], rtol=5e-4)
    np.testing.assert_allclose(gn[:5], fx["trace_gnorm"][:5], rtol=2e-3)
    np.testing.assert_allclose(loss, fx["trace_loss"][:n], rtol=5e-2)
    np.testing.assert_allclose(mu, fx["trace_mu"][:n], rtol=5e-3)
    eng.close()


@pytest.mark.parametrize("name", ["fx_nb_m0_g1_p3_32x4.npz", "fx_nb_m0_g1_p2_64x3.npz"])
def test_golden_notebook_trace(name):
    fx = H.load_fx(name)
    pb = H.problem_from_nb(fx)
    eng = make_engine(pb, fx["flat0"], fx["x"], H.bc_points(fx), lr=1e-3, sched=gpe_pinn.SCHED_PLATEAU)
    n = 20
    trace = [eng.step() for _ in range(n)]
    loss = np.array([t["loss"] for t in trace]); mu = np.array([t["mu"] for t in trace])
    np.testing.assert_allclose(loss[:8], fx["trace_loss"][:8], rtol=3e-3)
    np.testing.assert_allclose(mu[:8], fx["trace_mu"][:8], rtol=2e-3)
    np.testing.assert_allclose(loss, fx["trace_loss"][:n], rtol=8e-2)
    eng.close()


@pytest.mark.parametrize("name", H.refine_names())
def test_eval_density_refine(name):
    fx = H.load_fx(name)
    pb = H.problem_from_refine(fx)
    eng = make_engine(pb, fx["flat_final"], fx["x"], None)
    xt = fx["eval_x"]
    u, dens = eng.eval_density(torch.as_tensor(xt, device="cuda"), float(xt[1, 0] - xt[0, 0]),
                               abs_flag=(int(fx["mode"]) == 0))
    assert H.rel_err(u.cpu().numpy()[:, 0], fx["eval_u"]) < 5e-5
    eng.close()


def test_known_answer_zero_perturbation():
    """with zero perturbation u = phi_n exactly, so lambda = 2n+1 (refine convention) and pde_loss ~ 0,
    at BASELINE cfg2's full size (65 536 points)."""
    N = 65536
    x = np.linspace(-10, 10, N, dtype=np.float64).reshape(-1, 1)
    for mode in (0, 1, 4):
        pb = go.Problem(layers=[1, 64, 64, 64, 64, 1], activation=1, kinetic_coeff=1.0, pot_scale=1.0, gamma=0.0,
                        base_mode=mode, perturb_scale=0.0, dx=20.0 / (N - 1), w_bc=0.0)
        flat = np.random.default_rng(mode).normal(0, 0.2, go.param_count(pb.layers))
        eng = make_engine(pb, flat, x, None)
        sc, _, _ = eng.residual(want_fields=False)
        assert abs(sc["mu"] - (2 * mode + 1)) < 2e-5 * (2 * mode + 1)
        assert sc["pde"] < 1e-8
        assert abs(sc["integral"] - 1.0) < 1e-5
        eng.close()


def test_history_and_run_equivalence():
    kw = dict(layers=[1, 32, 32, 1], gamma=1.0, base_mode=0, dx=0.05)
    x, flat, x_bc = _inputs(kw, 256)
    pb = go.Problem(**kw)
    a = make_engine(pb, flat, x, x_bc)
    b = make_engine(pb, flat, x, x_bc)
    ta = [a.step() for _ in range(7)]
    b.run(7)
    hb = b.read_history(1, 7)
    for s, h in zip(ta, hb):
        assert abs(s["loss"] - h["loss"]) <= 1e-6 * abs(s["loss"]) and s["step"] == h["step"]
    assert np.abs(a.get_params() - b.get_params()).max() < 1e-6
    m, v, step = a.get_adam_state()
    assert step == 7 and np.isfinite(m).all() and (v >= 0).all()


def test_error_behaviour():
    with pytest.raises(ValueError):                                   # reference: ValueError("Unknown potential type")
        Engine(GPEConfig(layers=[1, 32, 32, 1], potential=17))
    with pytest.raises(ValueError):
        Engine(GPEConfig(layers=[4, 32, 32, 1]))
    with pytest.raises(ValueError):
        Engine(GPEConfig(layers=[2, 300, 300, 1], path=gpe_pinn.PATH_FUSED))          # no whole-network kernel for this width (> 256: not padded)
    e96 = Engine(GPEConfig(layers=[2, 96, 96, 1], path=gpe_pinn.PATH_FUSED))          # plain tanh: runs zero-padded to 128
    assert e96.active_path == gpe_pinn.PATH_FUSED and e96.n_params == 2 * 96 + 96 + 96 * 96 + 96 + 96 + 1
    e96.close()
    eng = Engine(GPEConfig(layers=[1, 32, 32, 1]))
    with pytest.raises(gpe_pinn.GPEError) as ei:
        eng.step()
    assert ei.value.code == gpe_pinn.capi.GPE_ERR_STATE
    with pytest.raises(gpe_pinn.GPEError):
        eng.set_params(np.zeros(5, np.float32))
    # non-finite loss: parameters must not move, status NONFINITE
    eng.set_params(np.full(eng.n_params, np.nan, np.float32))
    eng.bind_points(torch.zeros((16, 1), device="cuda"))
    before = eng.get_params()
    with pytest.raises(gpe_pinn.GPEError) as ei:
        eng.step()
    assert ei.value.code == gpe_pinn.capi.GPE_ERR_NONFINITE
    after = eng.get_params()
    assert np.array_equal(np.isnan(before), np.isnan(after))


def test_tanh_accuracy_through_forward():
    """The device tanh (gpe_common.h) against numpy over the whole useful range, via a 1-hidden-unit-wide network."""
    layers = [1, 32, 32, 1]
    P = go.param_count(layers)
    flat = np.zeros(P, np.float32)
    params = go.unflatten(flat, layers)
    # first layer: identity-ish scaling so that z spans [-12, 12]
    W0 = np.zeros((32, 1), np.float32); W0[:, 0] = np.linspace(0.01, 1.0, 32)
    params[0] = (W0, np.zeros(32, np.float32))
    W1 = np.eye(32, dtype=np.float32) * 3.0
    params[1] = (W1, np.zeros(32, np.float32))
    params[2] = (np.ones((1, 32), np.float32), np.zeros(1, np.float32))
    flat = go.flatten(params).astype(np.float32)
    x = np.linspace(-12, 12, 4097, dtype=np.float32).reshape(-1, 1)
    for path in ("generic", "fused"):
        eng = Engine(GPEConfig(layers=layers, path=PATHS[path]))
        eng.set_params(flat)
        got = eng.forward(torch.as_tensor(x, device="cuda")).cpu().numpy()
        ref, _ = go.mlp_forward(go.unflatten(flat.astype(np.float64), layers), x.astype(np.float64), 0, value_only=True)
        assert np.abs(got - ref[0]).max() < 2e-5          # sum of 32 tanh values, each good to ~3e-7
        eng.close()


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5])
def test_stored_reference_checkpoint_mu_table(mode):
    """The reference's stored trained weights (fx_ckpt_harmonic_modes.npz, from harmonic_mode_zero_plot_data.pkl) through the
    engine: lambda must match the mu_table the reference recorded (fp32 on both sides; tolerance 5e-5)."""
    fx = H.load_fx("fx_ckpt_harmonic_modes.npz")
    N = int(fx["N"])
    x = np.linspace(float(fx["lb"]), float(fx["ub"]), N).reshape(-1, 1)
    pb = go.Problem(layers=[int(v) for v in fx["layers"]], activation=1, kinetic_coeff=1.0, pot_scale=1.0, gamma=0.0, p=3,
                    base_mode=mode, perturb_scale=float(fx["perturb_const"]) / float(fx[f"const_mode{mode}"]),
                    dx=float(x[1, 0] - x[0, 0]), w_bc=0.0)
    for path in ("generic", "fused"):
        eng = make_engine(pb, fx[f"flat_mode{mode}"], x, None, path=PATHS[path])
        sc, _, _ = eng.residual(want_fields=False)
        assert abs(sc["mu"] - float(fx[f"mu_mode{mode}"])) < 5e-5, (path, sc["mu"])
        eng.close()


@pytest.mark.parametrize("name", ["fx_box_m0_g0.npz", "fx_box_m1_g20.npz"])
@pytest.mark.parametrize("path", ["generic", "fused"])
def test_golden_box_oplevel(name, path):
    """Row f3: box potential flavour (refine/box_pinn_simulation.py) -- engine vs the reference's own numbers and the oracle."""
    fx = H.load_fx(name)
    pb = H.problem_from_box(fx)
    xb = np.array([[0.0], [1.0]])
    eng = make_engine(pb, fx["flat0"], fx["x"], xb, path=PATHS[path])
    fwd = eng.forward(torch.as_tensor(fx["x"], device="cuda")).cpu().numpy()
    assert H.rel_err(fwd, fx["forward_out"]) < 1e-5                     # model.forward includes the sin(pi x) factor
    rs, psi, res = eng.residual()
    assert H.rel_err(psi.cpu().numpy(), fx["u"]) < 2e-6
    assert abs(rs["mu"] - float(fx["lam"])) < 5e-5 * abs(float(fx["lam"]))
    sc = eng.step()
    assert abs(sc["loss"] - float(fx["total"])) < 1e-3 * max(float(fx["total"]), 1e-4)
    osc, ograd, _ = go.full_loss_and_grad(pb, fx["flat0"].astype(np.float64), fx["x"].astype(np.float64), xb)
    assert H.rel_err(eng.get_grad(), ograd) < 5e-5
    assert H.rel_err(eng.get_grad(), fx["grad0"]) < 1e-3
    eng.close()


@pytest.mark.parametrize("mode", [0, 3])
def test_stored_box_checkpoint_mu_table(mode):
    fx = H.load_fx("fx_ckpt_box_modes.npz")
    x = np.linspace(0.0, 1.0, int(fx["N"])).reshape(-1, 1)
    pb = H.problem_from_box(fx, mode=mode, const=float(fx[f"const_mode{mode}"]))
    eng = make_engine(pb, fx[f"flat_mode{mode}"], x, None)
    sc, _, _ = eng.residual(want_fields=False)
    assert abs(sc["mu"] - float(fx[f"mu_mode{mode}"])) < 1e-4 * float(fx[f"mu_mode{mode}"])
    eng.close()


def test_precomputed_base_equals_analytic_base():
    """GPE_BASE_PRECOMPUTED (how the Airy base of refine/gravity_well_pinn_simulation.py enters): feeding the Hermite base as
    three arrays must reproduce the analytic-base step exactly."""
    kw = dict(layers=[1, 64, 64, 64, 1], activation=1, kinetic_coeff=1.0, pot_scale=1.0, gamma=3.0, base_mode=2,
              perturb_scale=0.05, dx=12 / 499)
    x, flat, x_bc = _inputs(kw, 500)
    pb = go.Problem(**kw)
    a = make_engine(pb, flat, x, None)
    sa = a.step(); ga = a.get_grad()
    phi, p1, p2 = go.hermite_base(x[:, 0].astype(np.float64), 2)
    b = make_engine(go.Problem(**{**kw, "base_kind": go.BASE_PRECOMPUTED}), flat, x, None)
    b.bind_base(phi, p1, p2)
    sb = b.step(); gb = b.get_grad()
    assert abs(sa["mu"] - sb["mu"]) < 1e-6 * abs(sa["mu"]) and abs(sa["loss"] - sb["loss"]) < 1e-5 * abs(sa["loss"])
    assert H.rel_err(gb, ga) < 1e-5


@pytest.mark.parametrize("name", ["fx_gravity_m0_g0.npz", "fx_gravity_m1_g5.npz"])
def test_golden_gravity_well_oplevel(name):
    """Row f3: gravity well (V = x, Airy base as precomputed arrays, boundary base folded into the target)."""
    fx = H.load_fx(name)
    pb = H.problem_from_gravity(fx)
    x = fx["x"]
    xb = np.array([[float(fx["lb"])], [float(fx["ub"])]], np.float32)
    for path in ("generic", "fused"):
        cfg = cfg_from_problem(pb, path=PATHS[path])
        eng = Engine(cfg)
        eng.set_params(fx["flat0"])
        eng.bind_points(torch.as_tensor(x, device="cuda"), V=torch.as_tensor(x[:, 0].copy(), device="cuda"))
        eng.bind_base(fx["base"][:, 0], fx["base_x"][:, 0], fx["base_xx"][:, 0])
        eng.bind_boundary(torch.as_tensor(xb, device="cuda"), torch.as_tensor(-fx["base_boundary"].astype(np.float32), device="cuda"))
        rs, psi, res = eng.residual()
        assert H.rel_err(psi.cpu().numpy(), fx["u"]) < 2e-6
        assert abs(rs["mu"] - float(fx["lam"])) < 5e-5 * abs(float(fx["lam"]))
        sc = eng.step()
        assert abs(sc["loss"] - float(fx["total"])) < 5e-4 * float(fx["total"])
        assert H.rel_err(eng.get_grad(), fx["grad0"]) < 1e-3
        eng.close()


@pytest.mark.parametrize("name", ["fx_paper_g10_p3.npz", "fx_paper_g2_p2.npz"])
@pytest.mark.parametrize("path", ["generic", "fused"])
def test_golden_paper_riesz_oplevel(name, path):
    """Row f4: Riesz energy term -- engine vs the Paper notebook's own numbers and the oracle."""
    fx = H.load_fx(name)
    pb = H.problem_from_paper(fx)
    eng = make_engine(pb, fx["flat0"], fx["x"], H.bc_points(fx), path=PATHS[path], w_riesz=pb.w_riesz)
    sc = eng.step()
    assert abs(sc["riesz"] - float(fx["riesz"])) < 2e-5 * abs(float(fx["riesz"]))
    assert abs(sc["loss"] - float(fx["total"])) < 2e-4 * float(fx["total"])
    osc, ograd, _ = go.full_loss_and_grad(pb, fx["flat0"].astype(np.float64), fx["x"].astype(np.float64), H.bc_points(fx))
    assert H.rel_err(eng.get_grad(), ograd) < 5e-5
    assert H.rel_err(eng.get_grad(), fx["grad0"]) < 5e-4
    # loss-weight setter (host-side balancers): doubling every weight doubles the gradient
    eng.set_params(fx["flat0"])
    eng.set_loss_weights(2 * pb.w_pde, 2 * pb.w_bc, 2 * pb.w_norm, 2 * pb.w_sym, 0.0, 2 * pb.w_riesz)
    sc2 = eng.step()
    assert abs(sc2["loss"] - 2 * osc["loss"]) < 2e-4 * 2 * osc["loss"]
    assert H.rel_err(eng.get_grad(), 2 * ograd) < 5e-5
    eng.close()


# ---- execution-mode switches of the engine give the same numbers --------------------------------------------------------------
def _trajectory(env, kw, N, steps, use_run):
    """(losses, final parameters) of `steps` steps on a fresh engine created under the environment `env`."""
    import os
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        x, flat, x_bc = _inputs(kw, N)
        eng = make_engine(go.Problem(**kw), flat, x, x_bc)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if use_run:
        eng.run(steps)
        losses = [h["loss"] for h in eng.read_history(1, steps)]
    else:
        losses = [eng.step()["loss"] for _ in range(steps)]
    theta = eng.get_params()
    grad = eng.get_grad()
    eng.close()
    return np.array(losses), theta, grad


@pytest.mark.parametrize("kw,N", [(dict(layers=[1, 64, 64, 64, 1], activation=1, gamma=5.0, base_mode=0, perturb_scale=0.05,
                                        dx=12 / 499), 500),
                                  (dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=0.01), 777)])
def test_side_stream_and_graph_replay_change_nothing(kw, N):
    """Boundary batch merged into the collocation batch (default when it is small) vs separate on the side stream vs separate in
    line (GPE_SIDE_STREAM=0), each with and without hipGraph replay of gpe_run (GPE_GRAPH=1):
    same kernels and arithmetic; the fused kernels accumulate weight gradients with LDS float atomics from several waves, so
    two runs agree to fp32 round-off, not bit for bit (the trajectories stay within 1e-5 over 12 steps)."""
    def same(a, b):
        return np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-5 * max(1.0, np.abs(np.asarray(b)).max())
    base_l, base_t, _ = _trajectory({"GPE_MERGE_BC": "0", "GPE_SIDE_STREAM": "0", "GPE_GRAPH": "0"}, kw, N, 12, use_run=True)
    for env in ({"GPE_MERGE_BC": "0", "GPE_SIDE_STREAM": "1", "GPE_GRAPH": "0"},
                {"GPE_MERGE_BC": "0", "GPE_SIDE_STREAM": "1", "GPE_GRAPH": "1"},
                {"GPE_MERGE_BC": "0", "GPE_SIDE_STREAM": "0", "GPE_GRAPH": "1"},
                {"GPE_MERGE_BC": "1", "GPE_GRAPH": "0"},          # boundary points appended to the collocation batch (default)
                {"GPE_MERGE_BC": "1", "GPE_GRAPH": "1"}):
        l, t, _ = _trajectory(env, kw, N, 12, use_run=True)
        assert same(l, base_l), env
        assert same(t, base_t), env
    l, t, _ = _trajectory({}, kw, N, 12, use_run=False)         # step-by-step with host synchronisation
    assert same(l, base_l) and same(t, base_t)


@pytest.mark.parametrize("kw,N,envs", [
    (dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=0.01), 4096,
     [{"GPE_COOP": "1", "GPE_COOP_FWD_MAX_TILES": "0"}, {"GPE_COOP": "1", "GPE_COOP_FWD_MAX_TILES": "1000000000"},
      {"GPE_COOP": "1", "GPE_COOP_FWD_MAX_TILES": "1000000000", "GPE_FUSE_HEAD": "0"},   # head by k_head_pde instead of inside the forward kernel
      {"GPE_COOP": "1", "GPE_PIPE": "0", "GPE_COOP_FWD_MAX_TILES": "0"},          # two-barrier cooperative reverse kernel
      {"GPE_COOP": "1", "GPE_FUSE_SEED": "0", "GPE_COOP_FWD_MAX_TILES": "0"},     # seeds by k_seed_pde instead of inside the reverse kernel
      {"GPE_COOP": "0", "GPE_STAGE_MIN_TILES": "0"}, {"GPE_COOP": "0", "GPE_STAGE_MIN_TILES": "1000000000"},
      {"GPE_COOP": "0", "GPE_STAGE_MIN_TILES": "0", "GPE_RACC": "0"}, {"GPE_COOP": "0", "GPE_WLDS": "0"}]),
    (dict(layers=[1, 32, 32, 32, 1], gamma=5.0, base_mode=0, dx=0.01), 1000,
     [{"GPE_COOP": "1"}, {"GPE_COOP": "1", "GPE_PIPE": "0"}, {"GPE_COOP": "1", "GPE_FUSE_SEED": "0"}, {"GPE_COOP": "1", "GPE_FUSE_HEAD": "0"},
      {"GPE_COOP": "0", "GPE_STAGE_MIN_TILES": "0"},
      {"GPE_COOP": "0", "GPE_STAGE_MIN_TILES": "1000000000"}]),
    (dict(layers=[2, 128, 128, 128, 1], gamma=50.0, dx=0.01), 777,
     [{"GPE_WIDE": "0", "GPE_COOP128": "1", "GPE_COOP_FWD128": "1"}, {"GPE_WIDE": "0", "GPE_COOP128": "0", "GPE_COOP_FWD128": "0"},
      {"GPE_WIDE": "0", "GPE_COOP128": "1", "GPE_COOP_FWD128": "0"}, {"GPE_WIDE_MIN_TILES": "0"}, {"GPE_WIDE": "1", "GPE_WIDE_MIN_TILES": "0"}]),
    # residual blocks: cooperative whole-network kernels with the skip connection, head in the forward kernel or in its own launch
    (dict(layers=[1, 64, 64, 64, 1], net_kind=go.NET_RESIDUAL, activation=1, kinetic_coeff=1.0, potential=go.POT_GAUSSIAN, pot_a=0.5, gamma=3.0,
          base_mode=0, perturb_scale=0.05, dx=0.01), 1000,
     [{}, {"GPE_FUSE_HEAD": "0"}]),
    # five hidden -> hidden maps at H = 64: cooperative kernels (default) against the unstaged per-wave-tile pair (GPE_COOP=0)
    (dict(layers=[2, 64, 64, 64, 64, 64, 64, 1], gamma=20.0, dx=0.01), 900,
     [{}, {"GPE_FUSE_HEAD": "0"}, {"GPE_COOP": "0"}]),
])
def test_kernel_variants_agree(kw, N, envs):
    """The fused path has several kernels for the same two primitives -- cooperative (a workgroup per tile), per-wave-tile with
    LDS-staged weights + register-resident gradients, per-wave-tile unstaged with LDS-atomic gradients, global-atomic slabs for
    H = 128, the wide set's per-map reverse kernels (default for H = 128 from 2 048 tiles on; GPE_WIDE_MIN_TILES=0 takes them at any size) -- selected by shape and batch size.  One step from the same state must agree to fp32 round-off whichever runs."""
    scale = _scale(kw)
    ref = None
    seen = set()
    for env in envs:
        import os
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            x, flat, x_bc = _inputs(kw, N, scale=scale)
            eng = make_engine(go.Problem(**kw), flat, x, x_bc)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        kern = eng.active_kernels
        seen.add((kern["fwd"], kern["bwd"]))
        sc = eng.step()
        g = eng.get_grad()
        eng.close()
        if ref is None:
            ref = (sc["loss"], g)
        else:
            assert abs(sc["loss"] - ref[0]) <= 2e-6 * abs(ref[0]), env
            assert H.rel_err(g, ref[1]) < 3e-6, env
    # every row ran a different kernel pair -- unless the suite itself runs under a forced switch (e.g. GPE_FWD_B6=1 GPE_BWD_B6=1 to
    # put the split-bf16 kernels through every test), which makes some rows coincide: then at least two distinct pairs
    import os
    forced = [k for k in ("GPE_FWD_B6", "GPE_BWD_B6", "GPE_PIPE", "GPE_COOP", "GPE_WIDE", "GPE_WIDE_MIN_TILES", "GPE_RES_FUSED", "GPE_COOP_FWD_MAX_TILES", "GPE_STAGE_MIN_TILES", "GPE_FUSE_SEED", "GPE_FUSE_HEAD")
              if k in os.environ]
    if forced:
        assert len(seen) >= 2, f"forced {forced}: switches selected only {sorted(seen)}"
    else:
        assert len(seen) == len(envs), f"switches selected only {sorted(seen)}"


@pytest.mark.parametrize("N", [4000, 50000])
def test_head_inside_the_forward_kernel_sums_in_a_fixed_order(N):
    """Whole steps of real-psi problems run the head inside the forward kernel (<= 6 144 points: f_forward_coop, >= 32 769: f_forward): one
    (sum u Hu, sum u^2, sum e_bc^2) triple per workgroup, added in a fixed order by the consumer -- so lambda and the norm integral of a
    step are reproducible bit for bit (the k_head_pde path adds with double atomics in arrival order), and agree with that path."""
    import os
    kw = dict(layers=[1, 64, 64, 64, 1], gamma=10.0, base_mode=0, dx=12.0 / (N - 1))
    x, flat, x_bc = _inputs(kw, N)
    runs = []
    for env in ({}, {}, {"GPE_FUSE_HEAD": "0"}):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            eng = make_engine(go.Problem(**kw), flat, x, x_bc)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        fwd = eng.active_kernels["fwd"]
        sc = [eng.step() for _ in range(3)]
        runs.append((fwd, [(r["mu"], r["num"], r["den"], r["integral"]) for r in sc]))
        eng.close()
    if not any(k in os.environ for k in ("GPE_FUSE_HEAD", "GPE_FWD_B6", "GPE_COOP", "GPE_COOP_FWD_MAX_TILES")):
        assert runs[0][0].endswith(",head>") and not runs[2][0].endswith(",head>"), [r[0] for r in runs]
        assert runs[0][1][0] == runs[1][1][0]                     # first step: identical bit for bit
    for a, b in zip(runs[0][1], runs[2][1]):
        assert abs(a[0] - b[0]) <= 2e-6 * abs(b[0]) and abs(a[2] - b[2]) <= 2e-6 * abs(b[2])


def test_uneven_tile_split_of_large_batches_changes_nothing_but_the_order():
    """Large batches on two workgroups per CU (f_forward, f_backward_pipe): the first-dispatched workgroup of a CU wins every arbitration
    and would finish early, so it is given 56 % / 62 % of the CU's tiles (GPE_PIPE_SHARE / GPE_FWD_SHARE, per 1024; 0 = even).  Which
    workgroup takes which tile only changes the order of the gradient sums: one step from the same state must agree to fp32 round-off."""
    import os
    kw = dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=0.01)
    N = 540000                                   # > 64 tiles per wave-pair of the forward kernel, ragged last tile
    scale = _scale(kw)
    x, flat, x_bc = _inputs(kw, N, scale=scale)
    out, names = [], []
    # (the last row also moves the head back into its own kernel: by default f_forward runs it from 32 769 points on)
    for env in ({}, {"GPE_PIPE_SHARE": "0", "GPE_FWD_SHARE": "0"}, {"GPE_PIPE_SHARE": "700", "GPE_FWD_SHARE": "300", "GPE_FUSE_HEAD": "0"}):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            eng = make_engine(go.Problem(**kw), flat, x, x_bc)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        names.append(eng.active_kernels["fwd"])
        sc = eng.step()
        out.append((sc["loss"], sc["mu"], eng.get_grad()))
        eng.close()
    if "GPE_FUSE_HEAD" not in os.environ and "GPE_FWD_B6" not in os.environ:
        assert names[0].endswith(",head>") and not names[2].endswith(",head>"), names
    for loss, mu, g in out[1:]:
        assert abs(loss - out[0][0]) <= 2e-6 * abs(out[0][0])
        assert abs(mu - out[0][1]) <= 2e-6 * abs(out[0][1])
        assert H.rel_err(g, out[0][2]) < 3e-6


def test_large_batch_launch_configuration_against_the_oracle():
    """The launch configuration of the headline run -- uneven tile split between the two workgroups of a CU in f_forward and
    f_backward_pipe, head inside the forward kernel, k_seed_pde adding the per-workgroup triples -- against the fp64 ORACLE itself
    (sharded two-phase evaluation), not against another kernel variant: 540 000 points (ragged last tile), one step."""
    import os
    kw = dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=0.01)
    N = 540000
    scale = _scale(kw)
    x, flat, x_bc = _inputs(kw, N, scale=scale)
    pb = go.Problem(**kw)
    eng = make_engine(pb, flat, x, x_bc)
    k = eng.active_kernels
    if not any(v in os.environ for v in ("GPE_PIPE_SHARE", "GPE_FWD_SHARE", "GPE_FUSE_HEAD", "GPE_FWD_B6", "GPE_PIPE", "GPE_COOP")):
        assert k["fwd"].endswith(",head>") and "f_backward_pipe" in k["bwd"] and k["split"] == "fwd 640/1024, bwd 576/1024", k
    sc = eng.step()
    g = eng.get_grad()
    eng.close()
    osc, ograd = go.sharded_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64),
                                          None if x_bc is None else x_bc.astype(np.float64), chunk=65536, threads=8)
    assert abs(sc["loss"] - osc["loss"]) <= 1e-4 * abs(osc["loss"]), (sc["loss"], osc["loss"])
    assert abs(sc["mu"] - osc["mu"]) <= 2e-5 * abs(osc["mu"]), (sc["mu"], osc["mu"])
    assert H.rel_err(g, ograd) < 5e-5


def test_large_batch_2d_class_loss_against_the_oracle():
    """The reference's 2D class loss (energy-functional lambda with its gradient branch, both regularisers, Riesz sum, 10 x boundary mean:
    src/gross_pitaevskii_2D.py:154-242) at a large batch -- 300 001 points in the disk, Gaussian potential handed over as an array, head and
    seed kernels in their own launches -- against the fp64 oracle (sharded evaluation): the double-precision point sums the lambda branch is
    made of hold at this size."""
    layers = [2, 64, 64, 64, 64, 1]
    N = 300001
    rng = np.random.default_rng(11)
    ang, rad = rng.uniform(0, 2 * np.pi, N), (np.pi / 2) * np.sqrt(rng.uniform(0, 1, N))
    x = np.stack([np.pi / 2 + rad * np.cos(ang), np.pi / 2 + rad * np.sin(ang)], 1).astype(np.float32)
    th = np.linspace(0, 2 * np.pi, 500)
    xb = np.stack([np.pi / 2 + (np.pi / 2) * np.cos(th), np.pi / 2 + (np.pi / 2) * np.sin(th)], 1).astype(np.float32)
    flat = (rng.normal(0, 1, go.param_count(layers)) * 0.3).astype(np.float32)
    pb = H.problem_from_class2d(dict(layers=np.array(layers), g=500.0))
    V = H.gaussian_2d(x.astype(np.float64))
    eng = Engine(cfg_from_problem(pb, clip_norm=0.0))
    eng.set_params(flat)
    eng.bind_points(torch.as_tensor(x, device="cuda"), V=torch.as_tensor(V.astype(np.float32), device="cuda"))
    eng.bind_boundary(torch.as_tensor(xb, device="cuda"))
    assert eng.active_path == gpe_pinn.PATH_FUSED and "head" not in eng.active_kernels["fwd"]
    sc = eng.step()
    g = eng.get_grad()
    eng.close()
    osc, ograd = go.sharded_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), xb.astype(np.float64), chunk=65536, threads=8,
                                          V_pre=V.astype(np.float32).astype(np.float64))
    for k, tol in (("loss", 1e-4), ("mu", 2e-5), ("riesz", 1e-4), ("reg", 1e-4), ("pde", 1e-4), ("bc", 1e-4)):
        assert abs(sc[k] - osc[k]) <= tol * abs(osc[k]), (k, sc[k], osc[k])
    assert H.rel_err(g, ograd) < 5e-5


@pytest.mark.parametrize("layers,sym,sched", [([1, 32, 32, 32, 32, 1], 5.0, go.SCHED_PLATEAU), ([1, 64, 64, 64, 1], 0.0, go.SCHED_COSINE_LOSS),
                                              ([2, 64, 64, 64, 64, 1], 0.0, go.SCHED_CONST)])
def test_update_kernel_forms_are_bit_identical(layers, sym, sched):
    """The single-workgroup update has two forms: elements cached in registers from the top of the kernel with the repacked weights
    SCATTERED from the Adam loop (default up to 13 312 parameters), and the two-pass form (GPE_UPDATE_CACHE=0: reload, then a gather
    pass that repacks).  Same arithmetic, same summation order: 30 steps must agree bit for bit -- which also proves the scatter
    addressing, since from the second step on every forward / reverse pass reads the scattered copies.  The multi-workgroup form
    (large P; forced here with GPE_UPDATE_MULTI_MIN=1) sums |g|^2 in another order: equal to rounding."""
    import os
    d = layers[0]
    N = 700
    rng = np.random.default_rng(3)
    x = (np.linspace(-8, 8, N).reshape(-1, 1) if d == 1 else rng.uniform(-4, 4, (N, d))).astype(np.float32)
    flat = (rng.normal(0, 0.3, go.param_count(layers))).astype(np.float32)
    kw = dict(layers=layers, gamma=1.0, p=3, base_mode=0 if d == 1 else -1, base_deriv=1, w_sym=sym, dx=16.0 / N, lr=1e-3, sched=sched)

    def run(env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            eng = Engine(GPEConfig(**kw))
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        eng.set_params(flat)
        eng.bind_points(torch.as_tensor(x, device="cuda"))
        if d == 1:
            eng.bind_boundary(torch.tensor([[-8.0], [8.0]], device="cuda"))
        tr = [eng.step()["loss"] for _ in range(30)]
        th = eng.get_params()
        eng.close()
        return np.array(tr), th

    one = {}                                                      # default: slab reduction + the single-workgroup update kernel
    la, ta = run(one)
    lb, tb = run(dict(one, GPE_UPDATE_CACHE="0"))
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(ta, tb)
    # round 4: the update inside the slab-reduction launch, in the workgroup that arrives last (k_reduce_update, opt-in GPE_FUSE_UPDATE=1;
    # taken when there is no symmetry batch).  Same operations, same order: bit for bit.
    lf, tf = run(dict(one, GPE_FUSE_UPDATE="1"))
    np.testing.assert_array_equal(la, lf)
    np.testing.assert_array_equal(ta, tf)
    lc, tc = run(dict(one, GPE_UPDATE_MULTI_MIN="1"))
    assert np.abs(lc - la).max() <= 1e-5 * np.abs(la).max() and np.abs(tc - ta).max() < 1e-5
    # round 4, opt-in GPE_SPLIT_UPDATE=1 (whole steps of small networks without a symmetry batch): slab reduction in the update's
    # partition (k_grad_reduce_part: gradient + partial |g|^2 + snapshot) and the update on 64 workgroups with the new weights scattered
    # into the packed copies -- |g|^2 and the slab sums are added in another order: equal to rounding, and repeatable bit for bit
    ld, td = run({"GPE_SPLIT_UPDATE": "1"})
    assert np.abs(ld - la).max() <= 1e-5 * np.abs(la).max() and np.abs(td - ta).max() < 1e-5
    ld2, td2 = run({"GPE_SPLIT_UPDATE": "1"})
    np.testing.assert_array_equal(ld, ld2)
    np.testing.assert_array_equal(td, td2)


# ---- orthogonality penalty (north star; no reference code: the oracle is the definition, tests/test_oracle_autograd.py) --------
ORTH_CASES = {
    "1d_two_modes": (dict(layers=[1, 64, 64, 64, 1], gamma=3.0, base_mode=2, w_orth=7.0, dx=12 / 799), 800, 2),
    "2d_one_mode": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, w_orth=3.0, dx=36 / 2000), 2000, 1),
    "2d_128_two_modes": (dict(layers=[2, 128, 128, 128, 1], gamma=50.0, w_orth=3.0, dx=36 / 500), 500, 2),
}


def _orth_modes(x, n_o, seed=9):
    """smooth stand-ins for lower eigenmodes on the points: Gaussians times low polynomials, O(1) amplitudes"""
    rng = np.random.default_rng(seed)
    r2 = (x.astype(np.float64) ** 2).sum(axis=1)
    out = []
    for j in range(n_o):
        c = rng.normal(0, 1, x.shape[1] + 1)
        out.append((c[0] + x.astype(np.float64) @ c[1:]) * np.exp(-0.5 * r2 / (1.0 + j)))
    return np.stack(out)


@pytest.mark.parametrize("name", sorted(ORTH_CASES))
@pytest.mark.parametrize("path", ["generic", "fused"])
def test_orthogonality_step_matches_oracle(name, path):
    kw, N, n_o = ORTH_CASES[name]
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    orth = _orth_modes(x, n_o)
    pb = go.Problem(**kw)
    osc, ograd, _ = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64), orth=orth)
    assert osc["orth"] > 1e-4 * osc["loss"]            # the term matters in this case
    eng = make_engine(pb, flat, x, x_bc, path=PATHS[path])
    for j in range(n_o):
        eng.bind_orth(j, orth[j].astype(np.float32))
    rs, _, _ = eng.residual()
    assert abs(rs["orth"] - osc["orth"]) <= 1e-4 * osc["orth"]
    sc = eng.step()
    for k, tol in (("mu", 2e-5), ("loss", 1e-4), ("orth", 1e-4), ("pde", 1e-4)):
        assert abs(sc[k] - osc[k]) <= tol * max(abs(osc[k]), 1e-6), (k, sc[k], osc[k])
    assert H.rel_err(eng.get_grad(), ograd) < 5e-5
    # unbinding restores the plain step
    for j in range(n_o):
        eng.bind_orth(j, None)
    eng.set_params(flat)
    o0, g0, _ = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64))
    sc0 = eng.step()
    assert sc0["orth"] == 0.0 and abs(sc0["loss"] - o0["loss"]) <= 1e-4 * abs(o0["loss"])
    assert H.rel_err(eng.get_grad(), g0) < 5e-5
    eng.close()


def test_orthogonality_shard_additivity_two_engines():
    """The S_ORTH sums ride in the first exchange: two engines on the two halves, buffers summed by hand, equal the full batch."""
    kw, N, n_o = ORTH_CASES["2d_one_mode"][0], 3001, 2
    x, flat, x_bc = _inputs(kw, N)
    orth = _orth_modes(x, n_o).astype(np.float32)
    pb = go.Problem(**kw, n_global=N)
    full = make_engine(pb, flat, x, x_bc)
    for j in range(n_o):
        full.bind_orth(j, orth[j])
    ref = full.step()
    gref = full.get_grad()
    lo = 1300
    engs = [make_engine(pb, flat, x[:lo], x_bc, world_size=2), make_engine(pb, flat, x[lo:], x_bc, world_size=2)]
    for e, sl in zip(engs, (slice(0, lo), slice(lo, N))):
        for j in range(n_o):
            e.bind_orth(j, orth[j][sl])
        e.step_begin()
    tot = engs[0].exchange_sums + engs[1].exchange_sums
    for e in engs:
        e.exchange_sums.copy_(tot)
        e.step_backward()
    gt = engs[0].exchange_grad + engs[1].exchange_grad
    for e in engs:
        e.exchange_grad.copy_(gt)
        e.step_update()
    for e in engs:
        sc = e.read_scalars()
        assert abs(sc["orth"] - ref["orth"]) <= 1e-5 * ref["orth"] and ref["orth"] > 0
        assert abs(sc["loss"] - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert H.rel_err(engs[0].get_grad(), gref) < 1e-5
    np.testing.assert_array_equal(engs[0].get_params(), engs[1].get_params())


# ---- d > 1 pinned by the reference's own 2D class, one point per call (tests/golden/make_golden_2d.py) -------------------------
@pytest.mark.parametrize("name", ["fx_2d_ref_points_64x4_g500.npz", "fx_2d_ref_points_100x3_g100.npz", "fx_2d_ref_points_128x5_g500.npz"])
def test_golden_2d_reference_points(name):
    """HIP jets (u, u_x, u_y, u_xx, u_yy) and H u = -lap u + V u + g u^3 against src/gross_pitaevskii_2D_minimal.py:170-182
    evaluated one point at a time (quirk Q1 inert).  The reference's Gaussian potential is handed over as a precomputed V."""
    fx = H.load_fx(name)
    layers = [int(v) for v in fx["layers"]]
    pb = go.Problem(layers=layers, kinetic_coeff=1.0, potential=go.POT_PRECOMPUTED, gamma=float(fx["g"]), p=3, dx=0.01)
    for path in ("generic", "fused"):            # (H = 100, the reference's own architecture: the fused path runs it padded to 128)
        eng = Engine(cfg_from_problem(pb, w_bc=0.0, path=PATHS[path]))
        eng.set_params(fx["flat0"])
        xt = torch.as_tensor(fx["x"], device="cuda")
        eng.bind_points(xt, V=torch.as_tensor(fx["V"].astype(np.float32), device="cuda"))
        jets = eng.forward_jets(xt).cpu().numpy()[:, :, 0]
        for c, key, tol in ((0, "u", 2e-6), (1, "u_x", 5e-6), (2, "u_y", 5e-6), (3, "u_xx", 2e-5), (4, "u_yy", 2e-5)):
            assert H.rel_err(jets[c], fx[key]) < tol, (path, key)
        sc, psi, res = eng.residual()
        Hu = res.cpu().numpy()[:, 0] + sc["mu"] * psi.cpu().numpy()[:, 0]          # r = H u - mu u
        assert H.rel_err(Hu, fx["residual"] + fx["lam"] * fx["u"]) < 3e-5, path
        eng.close()
        # riesz_loss of the same class on all points at once (src/gross_pitaevskii_2D_minimal.py:115-146; no broadcast quirk there)
        eng = Engine(cfg_from_problem(pb, w_bc=0.0, path=PATHS[path], w_riesz=1.0, riesz_kind=go.RIESZ_SUM))
        eng.set_params(fx["flat0"])
        eng.bind_points(xt, V=torch.as_tensor(fx["V"].astype(np.float32), device="cuda"))
        sc, _, _ = eng.residual()
        assert abs(sc["riesz"] - float(fx["riesz_all"])) < 2e-5 * abs(float(fx["riesz_all"])), path
        eng.close()


@pytest.mark.parametrize("name", H.CLASS2D)
def test_golden_2d_class_loss_and_gradient(name):
    """The 2D classes' whole loss (src/gross_pitaevskii_2D.py:215-242 = src/gross_pitaevskii_2D_minimal.py:201-222) through the C ABI, one
    collocation point per call like the golden generator (quirk Q1 inert): total, lambda (energy functional), pde + regularisers, Riesz sum,
    10 x boundary mean and the gradient of loss.backward(), on both kernel sets."""
    fx = H.load_fx(name)
    pb = H.problem_from_class2d(fx, n_global=1)
    layers = [int(v) for v in fx["layers"]]
    xb = torch.as_tensor(fx["x_bc"], device="cuda")
    for path in ("generic", "fused"):            # (H = 100: padded to 128 on the fused path)
        eng = Engine(cfg_from_problem(pb, path=PATHS[path], clip_norm=0.0))
        assert eng.active_path == PATHS[path]
        worst = 0.0
        for k in range(fx["x"].shape[0]):
            x = fx["x"][k:k + 1]
            eng.set_params(fx["flat0"])
            eng.reset_optimizer(1e-3)
            eng.bind_points(torch.as_tensor(x, device="cuda"), V=torch.as_tensor(H.gaussian_2d(x).astype(np.float32), device="cuda"))
            eng.bind_boundary(xb)
            sc = eng.step()
            # one point: lambda is a quotient by u^2 and the residual a cancelling sum -- fp32 round-off of the jets enters 10x amplified
            assert abs(sc["mu"] / fx["lam"][k] - 1) < 2e-4, (path, k, sc["mu"], fx["lam"][k])
            assert abs(sc["riesz"] / fx["riesz"][k] - 1) < 5e-5, (path, k)
            assert abs(10.0 * sc["bc"] / fx["bc_loss"][k] - 1) < 5e-5, (path, k)
            assert abs((sc["pde"] + sc["reg"]) / fx["pde_loss"][k] - 1) < 2e-3, (path, k, sc["pde"], sc["reg"], fx["pde_loss"][k])
            assert abs(sc["loss"] / fx["total"][k] - 1) < 5e-4, (path, k, sc["loss"], fx["total"][k])
            worst = max(worst, H.rel_err(eng.get_grad(), fx["grad"][k]))
        assert worst < 1e-3, (path, worst)
        eng.close()


# ---- generic set: VALU, 64x64-tile MFMA and 128x128-tile MFMA kernels are three implementations of the same maps ----------------
@pytest.mark.parametrize("kw,N", [(CASES["3d_256x6_cfg5_N4099"][0], 4099), (CASES["3d_128x6_N300"][0], 1500)])
def test_generic_kernel_variants_agree(kw, N):
    import os
    ref = None
    seen = set()
    for env in ({}, {"GPE_GEN_MFMA2": "0"}, {"GPE_GEN_MFMA": "0"}):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
            eng = make_engine(go.Problem(**kw), flat, x, x_bc, path=gpe_pinn.PATH_GENERIC)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        kern = eng.active_kernels
        seen.add((kern["fwd"], kern["bwd"]))
        sc = eng.step()
        g = eng.get_grad()
        eng.close()
        if ref is None:
            ref = (sc, g)
        else:
            assert abs(sc["loss"] - ref[0]["loss"]) <= 1e-5 * abs(ref[0]["loss"]), env
            assert abs(sc["mu"] - ref[0]["mu"]) <= 1e-5 * abs(ref[0]["mu"]), env
            assert H.rel_err(g, ref[1]) < 2e-5, env
    assert len(seen) == 3, sorted(seen)


def test_padded_hidden_widths_train_like_the_network_as_given():
    """Width padding (hidden widths without an MFMA kernel instance run zero-padded on the fused path): the padded weights must stay exactly
    zero under Adam, i.e. 40 steps on the padded network are 40 steps on the caller's network -- compared with the generic set, which takes
    the widths as given; parameters, gradient and Adam state cross the C ABI in the caller's layout and round-trip; GPE_PAD_WIDTH=0 keeps
    the generic set; ShiftedTanh networks are padded with units held at tanh = -1."""
    import os
    kw = dict(layers=[2, 100, 100, 100, 1], gamma=100.0, kinetic_coeff=1.0, pot_scale=1.0, dx=0.01)
    x, flat, x_bc = _inputs(kw, 1500, scale=0.15)
    pb = go.Problem(**kw)
    P = go.param_count(kw["layers"])
    a = make_engine(pb, flat, x, x_bc)                       # PATH_AUTO: padded, fused
    b = make_engine(pb, flat, x, x_bc, path=gpe_pinn.PATH_GENERIC)
    assert a.active_path == gpe_pinn.PATH_FUSED and b.active_path == gpe_pinn.PATH_GENERIC and a.n_params == b.n_params == P
    assert "padded" in a.active_kernels and "padded" not in b.active_kernels and a.exchange_grad.numel() > b.exchange_grad.numel()
    np.testing.assert_array_equal(a.get_params(), flat)
    for k in range(40):
        sa, sb = a.step(), b.step()
        if k < 5:                # (two kernel sets, two summation orders: clipped Adam amplifies the rounding from there on)
            assert abs(sa["loss"] - sb["loss"]) <= 1e-4 * (1 + k) * abs(sb["loss"]) and abs(sa["mu"] - sb["mu"]) <= 1e-4 * (1 + k) * abs(sb["mu"]), k
        if k == 0:
            assert H.rel_err(a.get_grad(), b.get_grad()) < 5e-5
    pa = a.get_params()
    assert np.abs(pa - flat).max() > 5e-3                                            # moved by ~40 lr
    # had a padded weight moved, the network function would no longer be the caller's: evaluate the returned parameters on the other set
    xt = torch.as_tensor(x, device="cuda")
    ua = a.forward(xt).cpu().numpy()
    b.set_params(pa)
    assert H.rel_err(b.forward(xt).cpu().numpy(), ua) < 2e-6
    m, v, step = a.get_adam_state()
    assert step == 40 and m.shape == (P,) and np.abs(m).max() > 0
    a.set_adam_state(m, v, step)
    m2, v2, step2 = a.get_adam_state()
    np.testing.assert_array_equal(m, m2); np.testing.assert_array_equal(v, v2)
    a.close(); b.close()
    os.environ["GPE_PAD_WIDTH"] = "0"
    try:
        c = make_engine(pb, flat, x, x_bc)
        assert c.active_path == gpe_pinn.PATH_GENERIC
        c.close()
    finally:
        os.environ.pop("GPE_PAD_WIDTH")
    # ShiftedTanh (tanh + 1): the padded units carry the bias -40, tanh = -1 exactly, output 0 with zero slope -- same contract
    pbs = go.Problem(**dict(kw, activation=1))
    d = make_engine(pbs, flat, x, x_bc)
    g = make_engine(pbs, flat, x, x_bc, path=gpe_pinn.PATH_GENERIC)
    assert d.active_path == gpe_pinn.PATH_FUSED and "padded" in d.active_kernels and g.active_path == gpe_pinn.PATH_GENERIC
    for k in range(30):
        sd, sg = d.step(), g.step()
        if k < 4:
            assert abs(sd["loss"] - sg["loss"]) <= 1e-4 * (1 + k) * abs(sg["loss"]), k
        if k == 0:
            assert H.rel_err(d.get_grad(), g.get_grad()) < 5e-5
    pd = d.get_params()
    g.set_params(pd)
    assert H.rel_err(g.forward(xt).cpu().numpy(), d.forward(xt).cpu().numpy()) < 1e-5 and np.abs(pd - flat).max() > 5e-3    # (a moved padding unit would show at 1e-2)
    d.close(); g.close()
    # widths above 256 (train_pinn's default [2,400,400,400,1]): padded to a multiple of 256 so that the GENERIC set runs its MFMA kernels
    kw2 = dict(layers=[2, 400, 400, 400, 1], gamma=100.0, kinetic_coeff=1.0, pot_scale=1.0, dx=0.01)
    x2, flat2, xb2 = _inputs(kw2, 700, scale=0.08)
    pb2 = go.Problem(**kw2)
    ea = make_engine(pb2, flat2, x2, xb2)
    eb = make_engine(pb2, flat2, x2, xb2, path=gpe_pinn.PATH_GENERIC)
    assert ea.active_path == gpe_pinn.PATH_GENERIC and "padded" in ea.active_kernels and "mfma" in ea.active_kernels["fwd"]
    assert "padded" not in eb.active_kernels and ea.n_params == eb.n_params == go.param_count(kw2["layers"])
    sa, sb = ea.step(), eb.step()
    assert abs(sa["loss"] - sb["loss"]) <= 2e-5 * abs(sb["loss"]) and abs(sa["mu"] - sb["mu"]) <= 2e-5 * abs(sb["mu"])
    assert H.rel_err(ea.get_grad(), eb.get_grad()) < 5e-5
    osc, ograd, _ = go.full_loss_and_grad(pb2, flat2.astype(np.float64), x2.astype(np.float64), xb2.astype(np.float64))
    assert abs(sa["loss"] - osc["loss"]) <= 1e-4 * abs(osc["loss"]) and H.rel_err(ea.get_grad(), ograd) < 5e-5
    ea.close(); eb.close()


# ---- native exchange: the engine's own RCCL communicator (world 1 on the one-GPU box: the same code path as N ranks) -----------
_CLASS_LOSS = dict(kinetic_coeff=1.0, pot_scale=1.0, w_norm=0.0, w_riesz=0.05, riesz_kind=go.RIESZ_SUM, lambda_kind=go.LAMBDA_ENERGY, w_reg_f=1.0,
                   w_reg_lam=1.0)
# the bucket-per-map exchange overlapped with the reverse pass exists on the generic set only: residual blocks, the H = 256 energy-functional
# lambda, complex psi with the variational energy and a single hidden layer step through it too, each also against the fp64 oracle
NATIVE_CASES = ["1d_residual_64x2blocks", "3d_energy_lambda_p5_256x2", "2d_complex_rot_variational", "1d_single_hidden"]


@pytest.mark.parametrize("path,extra,case", [("generic", {}, None), ("fused", {}, None), ("generic", _CLASS_LOSS, None), ("fused", _CLASS_LOSS, None)]
                         + [("generic", None, c) for c in NATIVE_CASES],
                         ids=["generic-north_star_loss", "fused-north_star_loss", "generic-2d_class_loss", "fused-2d_class_loss"]
                         + [f"generic-{c}" for c in NATIVE_CASES])
def test_native_rccl_step_equals_plain_step(path, extra, case):
    if case is None:
        kw = dict(layers=[2, 64, 64, 64, 1], gamma=50.0, dx=0.01, **extra)
        x, flat, x_bc = _inputs(kw, 3000)
    else:
        kw, N, _ = CASES[case]
        x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    a = make_engine(pb, flat, x, x_bc, path=PATHS[path])
    b = make_engine(pb, flat, x, x_bc, path=PATHS[path])
    assert b.active_path == PATHS[path]
    b.comm_init(0, 1)
    assert b.comm_info()["world"] == 1 and a.comm_info()["world"] == 0
    for k in range(3):
        a.step()
        b.step_dp()
        if k == 0 and case is not None:                # the first step over the communicator against the fp64 oracle (test_step_matches_oracle's bounds)
            osc, ograd, _ = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64))
            sc, grad = b.read_scalars(), b.get_grad()
            for key, tol in (("mu", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("bc", 1e-4), ("norm", 2e-4), ("sym", 1e-4), ("riesz", 1e-4), ("reg", 1e-4)):
                assert abs(sc[key] - osc[key]) <= tol * max(abs(osc[key]), 1e-6), (key, sc[key], osc[key])
            assert H.rel_err(grad, ograd) < 5e-5
            worst = H.block_rel_errs(grad, ograd, H.param_blocks(pb.layers, pb.net_kind))
            assert max(worst.values()) < 5e-5, worst
            assert abs(sc["grad_norm"] - np.linalg.norm(ograd)) < 1e-4 * np.linalg.norm(ograd)
            new, _, _ = go.optimizer_step(go.OptState(lr0=1e-3), flat, ograd, osc["loss"])
            d = np.abs(b.get_params() - new)
            assert np.quantile(d, 0.99) < 2e-5 and d.max() < 2.1e-3
    sa, sb = a.read_scalars(), b.read_scalars()
    assert abs(sa["loss"] - sb["loss"]) <= 1e-6 * abs(sa["loss"]) and abs(sa["mu"] - sb["mu"]) <= 1e-6 * abs(sa["mu"])
    assert np.abs(a.get_params() - b.get_params()).max() < 1e-6
    n = b.comm_info()["collectives"]
    # fused: sums + one gradient message per step; generic: sums + one bucket per linear map + the tail
    n_maps = len(go.expand_layers(kw["layers"], kw.get("net_kind", go.NET_MLP))[0]) - 1
    assert n == (3 * 2 if path == "fused" else 3 * (1 + n_maps + 1)), n
    with pytest.raises(gpe_pinn.GPEError):
        a.step_dp()                                   # no communicator: loud
    a.close(); b.close()


# ---- BASELINE configs[2..4] at their PER-GPU size: the two kernel sets are independent implementations; sums and gradients must
#      agree at full size (size-independent cross-check; the oracle pins the same shapes at small N in test_step_matches_oracle) --------
FULL_SIZE = {
    "cfg3_2d_5x128_131072": (dict(layers=[2, 128, 128, 128, 128, 128, 1], gamma=500.0), (512, 256), 8.0),
    "cfg4_2d_6x128_rot_262144": (dict(layers=[2, 128, 128, 128, 128, 128, 128, 2], gamma=500.0, complex_psi=True, omega_rot=0.8),
                                 (512, 512), 8.0),
    "cfg5_3d_6x256_524288": (dict(layers=[3, 256, 256, 256, 256, 256, 256, 1], gamma=1000.0, omega=(1.0, 1.4, 2.0)), (64, 128, 64), 6.0),
}


@pytest.mark.parametrize("name", sorted(FULL_SIZE))
def test_fused_and_generic_agree_at_per_gpu_size(name):
    kw, grid, half = FULL_SIZE[name]
    axes = [np.linspace(-half, half, n, dtype=np.float32) for n in grid]
    x = np.stack([m.ravel() for m in np.meshgrid(*axes, indexing="ij")], axis=1)
    dx = float(np.prod([2 * half / (n - 1) for n in grid]))
    rng = np.random.default_rng(2)
    flat = (rng.normal(0, 1, go.param_count(kw["layers"])) * _scale(kw)).astype(np.float32)
    pb = go.Problem(**kw, dx=dx)
    outs = {}
    for path in ("generic", "fused"):
        eng = make_engine(pb, flat, x, None, path=PATHS[path])
        sc = eng.step()
        outs[path] = (sc, eng.get_grad())
        eng.close()
        torch.cuda.empty_cache()
    (a, ga), (b, gb) = outs["generic"], outs["fused"]
    assert abs(a["mu"] - b["mu"]) < 1e-5 * abs(a["mu"])
    assert abs(a["loss"] - b["loss"]) < 1e-4 * abs(a["loss"])
    assert H.rel_err(gb, ga) < 3e-4


# ---- row f3: residual-block network flavour against numbers from the reference's own class (tests/golden/make_golden_box2gauss.py) ----
@pytest.mark.parametrize("path", ["generic", "fused"])
@pytest.mark.parametrize("name", ["fx_box2gauss_m0_g0.npz", "fx_box2gauss_m1_g5_p4.npz"])
def test_golden_box_to_gaussian_residual_network(name, path):
    """(round 4: the residual network runs on the cooperative whole-network kernels by default -- `fused` -- and on the generic set when asked)"""
    fx = H.load_fx(name)
    pb = H.problem_from_box2gauss(fx)
    xb = np.array([[float(fx["lb"])], [float(fx["ub"])]])
    if path == "fused" and len(pb.layers) - 3 > 2:          # three blocks: no whole-network kernel (one or two), the forced path says so
        with pytest.raises(ValueError):
            make_engine(pb, fx["flat0"], fx["x"], xb, path=PATHS[path])
        return
    eng = make_engine(pb, fx["flat0"], fx["x"], xb, path=PATHS[path])
    assert eng.active_path == PATHS[path]
    if path == "fused":
        auto = make_engine(pb, fx["flat0"], fx["x"], xb)
        assert auto.active_path == gpe_pinn.PATH_FUSED and "coop" in auto.active_kernels["bwd"]
        auto.close()
    fwd = eng.forward(torch.as_tensor(fx["x"], device="cuda")).cpu().numpy()
    assert H.rel_err(fwd, fx["forward_out"]) < 1e-5
    jets = eng.forward_jets(torch.as_tensor(fx["x"], device="cuda")).cpu().numpy()
    s = pb.perturb_scale
    base = go.base_functions(pb, fx["x"][:, 0].astype(np.float64))
    assert H.rel_err(s * jets[1][:, 0] + base[1], fx["u_x"][:, 0]) < 1e-5 and H.rel_err(s * jets[2][:, 0] + base[2], fx["u_xx"][:, 0]) < 1e-4
    rs, psi, res = eng.residual()
    assert H.rel_err(psi.cpu().numpy(), fx["u"]) < 2e-6
    assert abs(rs["mu"] - float(fx["lam"])) < 5e-5 * abs(float(fx["lam"]))
    sc = eng.step()
    assert abs(sc["loss"] - float(fx["total"])) < 1e-3 * float(fx["total"])
    osc, ograd, _ = go.full_loss_and_grad(pb, fx["flat0"].astype(np.float64), fx["x"].astype(np.float64), xb)
    assert H.rel_err(eng.get_grad(), ograd) < 5e-5
    assert H.rel_err(eng.get_grad(), fx["grad0"]) < 1e-3
    eng.close()
    # the class surface: same state_dict keys as the reference's nn.Sequential of ResidualBlocks
    from gpe_pinn import box_to_gaussian as b2g
    m = b2g.GrossPitaevskiiPINN([int(v) for v in fx["layers"]], mode=int(fx["mode"]), gamma=float(fx["gamma"]), L=float(fx["ub"]))
    assert list(m.state_dict().keys()) == [str(k) for k in fx["state_dict_keys"]]
    m.close()


@pytest.mark.parametrize("path", ["generic", "fused"])
def test_stale_gradient_mode_is_the_one_step_delayed_trajectory(path):
    """gpe_comm_set_async (opt-in): theta_{t+1} = Adam(theta_t, g(theta_{t-1})), step 0 applies nothing.  Emulated with the oracle:
    same clip / Adam, gradients taken one step late.  (World 1 through the native communicator: the code path of N ranks.)"""
    kw = dict(layers=[2, 64, 64, 64, 1], gamma=50.0, dx=0.01)
    x, flat, x_bc = _inputs(kw, 1500)
    pb = go.Problem(**kw)
    eng = make_engine(pb, flat, x, x_bc, path=PATHS[path])
    eng.comm_init(0, 1)
    eng.comm_set_async(True)
    K = 5
    for _ in range(K):
        eng.step_dp()
    eng.synchronize()
    got = eng.get_params()
    theta = flat.copy()
    st = go.OptState(lr0=1e-3)
    pend = None
    for t in range(K):
        sc, g, _ = go.full_loss_and_grad(pb, theta.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64))
        if pend is not None:
            theta, _, _ = go.optimizer_step(st, theta, pend[0], pend[1])
        pend = (g, sc["loss"])
    assert np.abs(got - theta).max() < 5e-5, np.abs(got - theta).max()
    # and it differs from the synchronous trajectory (which applies K updates, not K - 1)
    ref = make_engine(pb, flat, x, x_bc, path=PATHS[path])
    for _ in range(K):
        ref.step()
    assert np.abs(ref.get_params() - got).max() > 1e-4
    eng.close(); ref.close()


@pytest.mark.parametrize("name", ["2d_128x5_cfg3", "2d_128x6_complex_cfg4", "1d_128x2", "2d_complex_72x3_pads_to_128", "2d_128x3_cfg3like"])
def test_per_map_reverse_pass_of_h128_at_small_batches_matches_oracle(name):
    """H = 128 in 1D / 2D: batches under 2 048 tiles take the single-launch cooperative reverse kernel by default (test_step_matches_oracle
    covers that), larger ones the per-map kernels w_bwd_map<128> -- which GPE_WIDE_MIN_TILES=0 selects at any size, so that they too meet
    the oracle on the small cases the oracle can do (their full-size runs are cross-checked against the generic set)."""
    import os
    kw, N, _ = CASES[name]
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    osc, ograd, _ = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64))
    old = os.environ.get("GPE_WIDE_MIN_TILES")
    os.environ["GPE_WIDE_MIN_TILES"] = "0"
    try:
        eng = make_engine(pb, flat, x, x_bc)
    finally:
        os.environ.pop("GPE_WIDE_MIN_TILES", None) if old is None else os.environ.__setitem__("GPE_WIDE_MIN_TILES", old)
    assert "w_bwd_map<128" in eng.active_kernels["bwd"], eng.active_kernels
    sc = eng.step()
    assert abs(sc["loss"] - osc["loss"]) <= 1e-4 * abs(osc["loss"]) and abs(sc["mu"] - osc["mu"]) <= 2e-5 * abs(osc["mu"])
    assert H.rel_err(eng.get_grad(), ograd) < 5e-5
    eng.close()


def test_wide_set_output_layer_fused_or_separate_agree():
    """The topmost w_bwd_map launch forms zbar_{L-1}, dW_out, db_out itself (default) or reads what w_bwd_out wrote (GPE_WIDE_TOP=0)."""
    import os
    kw, N = CASES["3d_256x6_cfg5_N300"][0], 1100
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    res = []
    for top in ("1", "0"):
        old = os.environ.get("GPE_WIDE_TOP")
        os.environ["GPE_WIDE_TOP"] = top
        try:
            eng = make_engine(go.Problem(**kw), flat, x, x_bc, path=gpe_pinn.PATH_FUSED)
            sc = eng.step()
            res.append((sc["loss"], eng.get_grad()))
            eng.close()
        finally:
            os.environ.pop("GPE_WIDE_TOP", None) if old is None else os.environ.__setitem__("GPE_WIDE_TOP", old)
    assert abs(res[0][0] - res[1][0]) <= 1e-6 * abs(res[0][0])
    assert H.rel_err(res[0][1], res[1][1]) < 3e-6


@pytest.mark.parametrize("mode", ["fwd", "bwd", "both"])
@pytest.mark.parametrize("name", ["2d_64x4_g500", "1d_64x3_refine", "1d_32x4_nb_sym", "3d_64x3_aniso", "2d_64x3_complex_rot", "2d_N17_ragged"])
def test_split_bf16_kernels_match_oracle(name, mode):
    """GPE_FWD_B6=1 / GPE_BWD_B6=1 (opt-in): the H x H maps of the large-batch forward kernel (f_forward_b6) and the adjoint products of
    the cooperative reverse kernel (f_backward_coop<..., B6>) as six bf16 matrix products per fp32 product (three bf16 pieces per operand,
    fp32 accumulation).  Same tolerances as the fp32-MFMA kernels: the split keeps 24 significant bits."""
    import os
    kw, N, _ = CASES[name]
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    osc, ograd, ores = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64))
    old = {k: os.environ.get(k) for k in ("GPE_FWD_B6", "GPE_BWD_B6", "GPE_COOP_FWD_MAX_TILES")}
    os.environ["GPE_FWD_B6"] = "1" if mode in ("fwd", "both") else "0"
    os.environ["GPE_BWD_B6"] = "1" if mode in ("bwd", "both") else "0"
    os.environ["GPE_COOP_FWD_MAX_TILES"] = "0"          # small batches would take the cooperative forward kernel
    try:
        eng = make_engine(pb, flat, x, x_bc, path=gpe_pinn.PATH_FUSED)
        kern = eng.active_kernels
        assert kern["fwd"].startswith("f_forward_b6<") == (mode in ("fwd", "both"))
        assert kern["bwd"].endswith(",b6>") == (mode in ("bwd", "both")), kern
        rs, psi, res = eng.residual()
        assert close(psi.cpu().numpy(), ores["psi"], 5e-6, 2e-6)
        assert close(res.cpu().numpy(), ores["residual"], 2e-5, 1e-5)
        sc = eng.step()
        f = 10.0 if N < 4 else 1.0
        for k, tol in (("mu", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("norm", 2e-4)):
            assert abs(sc[k] - osc[k]) <= f * tol * max(abs(osc[k]), 1e-6), (k, sc[k], osc[k])
        assert H.rel_err(eng.get_grad(), ograd) < f * 5e-5
        eng.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.mark.parametrize("name", H.vbeta_names())
def test_golden_vary_beta_oplevel(name):
    """Row f3, beta-sweep flavours (refine/vary_potential_parameter_{harmonic,gravity_well,box_and_gaussian}.py): both kernel sets against
    the tensors of the reference's own classes -- u, lambda, total loss, gradient of the epoch-0 body."""
    fx = H.load_fx(name)
    pb, arr = H.problem_from_vbeta(fx)
    x = fx["x"]
    xb = np.array([[float(fx["lb"])], [float(fx["ub"])]], np.float32)
    for path in ("generic", "fused"):
        eng = Engine(cfg_from_problem(pb, path=PATHS[path]))
        eng.set_params(fx["flat0"])
        V = arr.get("V_pre")
        eng.bind_points(torch.as_tensor(x, device="cuda"), V=None if V is None else torch.as_tensor(V.astype(np.float32), device="cuda"))
        if "base_pre" in arr:
            eng.bind_base(*arr["base_pre"])
        tgt = arr.get("bc_target")
        eng.bind_boundary(torch.as_tensor(xb, device="cuda"), None if tgt is None else torch.as_tensor(tgt.astype(np.float32), device="cuda"))
        rs, psi, res = eng.residual()
        assert H.rel_err(psi.cpu().numpy(), fx["u"]) < 2e-6
        assert abs(rs["mu"] - float(fx["lam"])) < 5e-5 * abs(float(fx["lam"]))
        sc = eng.step()
        assert abs(sc["loss"] - float(fx["total"])) < 1e-3 * float(fx["total"])
        assert H.rel_err(eng.get_grad(), fx["grad0"]) < 1e-3
        eng.close()


def test_multi_tile_wide_forward_kernel_matches_oracle():
    """w_forward_mt (H = 128, several point tiles per pass; opt-in GPE_WIDE=1 GPE_WIDE_FWD_MT=1 -- measured slower than the defaults, kept as a
    recorded experiment): the H = 128 oracle cases through it, in a child process (the wide unit reads its switch once per process);
    N = 300 / 1000 give ragged last passes for TP = 3 and 4."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GPE_WIDE="1", GPE_WIDE_FWD_MT="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-q", "-m", "gpu", "-x",
                        "-k", "test_step_matches_oracle and 128 and fused"], capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


def test_randomised_parity_sweep():
    """tools/fuzz_parity.py, 120 random problem descriptions (dimension, hidden widths native / odd / ragged / above 256, depth, activation, residual
    blocks, complex psi, Riesz forms, energy-functional lambda, regularisers, symmetry, 7 .. 3 000 points) through whatever kernel set gpe_create
    picks, against the fp64 oracle: loss 2e-4, mu 5e-5, gradient 1e-4.  (1 200 cases from one point up: profiles/r04/fuzz_parity.txt.)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), "120", "3", "7"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
    # ... and 40 more, five steps each, also stepped data-parallel at world 3 on random uneven cuts with a 1-point shard (the tool's thresholds)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), "40", "5", "7", "1", "dp", "3"], capture_output=True, text=True,
                       timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]

