#!/usr/bin/env python3
"""Trains a 1D two-component mixture (gpe_config.mixture) to its ground state by continuation in the couplings and MEASURES the error.

Symmetric case: g11 = g22 = g, g12 < g, n_a = 1/2 in the trap V = x^2 / 2 (c = 1/2).  The symmetric state is u_1 = u_2 = phi / sqrt(2)
with phi the ground state of the scalar problem at g_eff = (g + g12) / 2 and mu_a = mu(g_eff): compared with oracle/gp_ground_state.py
(fp64 Newton solver) -- mu_1, mu_2 and both densities on the training grid.  Immiscible case (g12^2 > g11 g22): reported without a bar
(mu_a, norms, overlap of the densities): no reference state is claimed for it.

The network starts from a pre-training on the Gaussian of the linear problem (gpe_mse_step); then stages of plain steps, the couplings
raised stage by stage with gpe_set_mixture.  --energy W trains with the mixture energy term at weight W (gpe_mixture_energy_weight) and
records E of both runs (gpe_mixture_energy) next to the energies of the symmetric and the separated stationary state of the immiscible
couplings from the fp64 gradient flow tests/mixture_flow_1d.py.
usage: tools/accuracy_mixture.py [--energy W] [--out profiles/mixture_energy/accuracy_mixture_1d.json]"""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpe_pinn
from bench import reference_init
from oracle import gp_ground_state as gs

ap = argparse.ArgumentParser()
ap.add_argument("--g", type=float, default=10.0)
ap.add_argument("--g12", type=float, default=6.0)
ap.add_argument("--g12-immiscible", type=float, default=14.0)
ap.add_argument("--points", type=int, default=1024)
ap.add_argument("--half", type=float, default=8.0)
ap.add_argument("--stages", type=int, default=8)
ap.add_argument("--steps", type=int, default=4000, help="steps per continuation stage")
ap.add_argument("--pretrain", type=int, default=3000)
ap.add_argument("--energy", type=float, default=0.0, help="weight of the mixture energy term (0: residual loss alone)")
ap.add_argument("--out", default=None)
a = ap.parse_args()

layers, N, L = [1, 64, 64, 64, 2], a.points, a.half
x = np.linspace(-L, L, N, dtype=np.float64).reshape(-1, 1)
dx = 2 * L / (N - 1)
xd = torch.as_tensor(x.astype(np.float32), device="cuda")
xb = torch.as_tensor(np.array([[-L], [L]], np.float32), device="cuda")


def train(g11, g22, g12_end, norms, tilt):
    """-> (engine, seconds): pre-training on sqrt(n_a) x the linear ground state (tilt: the two components displaced by -/+ tilt, the seed
    an immiscible state needs to leave the symmetric saddle), then the couplings raised linearly over the stages"""
    cfg = gpe_pinn.GPEConfig(layers=layers, kinetic_coeff=0.5, pot_scale=0.5, dx=dx, w_pde=1.0, w_bc=10.0, w_norm=20.0, lr=1e-3, clip_norm=1.0,
                             mixture=True, mix_g=(0.0, 0.0, 0.0), mix_norm=norms, n_global=N)
    eng = gpe_pinn.Engine(cfg)
    eng.set_params(reference_init(layers, seed=1))
    eng.bind_points(xd); eng.bind_boundary(xb)
    tgt = np.stack([np.sqrt(norms[k]) * np.pi ** -0.25 * np.exp(-0.5 * (x[:, 0] + (tilt if k == 0 else -tilt)) ** 2) for k in range(2)], axis=1)
    eng.bind_target(torch.as_tensor(tgt.astype(np.float32), device="cuda"))
    t0 = time.time()
    for _ in range(a.pretrain):
        eng.mse_step()
    eng.reset_optimizer(1e-3)
    eng.set_mixture_energy(a.energy)
    for s in range(1, a.stages + 1):
        f = s / a.stages
        eng.set_mixture(f * g11, f * g22, f * g12_end)
        if s == a.stages:
            eng.set_lr(2e-4)
        eng.run(a.steps)
    eng.synchronize()
    return eng, time.time() - t0


def state(eng):
    sc, psi, res = eng.residual()
    return sc, eng.mixture_scalars(), psi.cpu().numpy().astype(np.float64), res.cpu().numpy().astype(np.float64)


rec = dict(tool="tools/accuracy_mixture.py", energy_weight=a.energy, layers=layers, points=N, box=[-L, L], dx=dx, stages=a.stages, steps_per_stage=a.steps, pretrain=a.pretrain)
# ---- symmetric, miscible: against the scalar solver at g_eff ----
g_eff = 0.5 * (a.g + a.g12)
lam, states = gs.ground_state_1d([g_eff], c=0.5, vscale=0.5, half=12.0)
xs, phi = states[g_eff]
phi_on_x = np.interp(x[:, 0], xs, phi)
eng, secs = train(a.g, a.g, a.g12, (0.5, 0.5), 0.0)
sc, m, u, r = state(eng)
E_miscible = eng.mixture_energy()["E"]
dens_ref = 0.5 * phi_on_x ** 2
sym = dict(g=a.g, g12=a.g12, g_eff=g_eff, mu_ref=lam[g_eff], mu1=m["mu1"], mu2=m["mu2"], mu1_abs_err=abs(m["mu1"] - lam[g_eff]),
           mu2_abs_err=abs(m["mu2"] - lam[g_eff]), integral1=m["integral1"], integral2=m["integral2"], loss=sc["loss"], pde=sc["pde"],
           density_max_abs_err=[float(np.abs(u[:, k] ** 2 / (m[f"integral{k + 1}"] / 0.5) - dens_ref).max()) for k in range(2)],
           density_peak_ref=float(dens_ref.max()), residual_rms=[float(np.sqrt(dx * (r[:, k] ** 2).sum())) for k in range(2)], train_seconds=secs)
sym["E"] = E_miscible
rec["symmetric"] = sym
eng.close()
# ---- immiscible: reported, no bar ----
eng, secs = train(a.g, a.g, a.g12_immiscible, (0.5, 0.5), 0.5)
sc, m, u, r = state(eng)
from tests import mixture_flow_1d as mf
E_sym, E_sep = mf.sym_and_sep(a.g, a.g12_immiscible)
d1, d2 = u[:, 0] ** 2, u[:, 1] ** 2
rec["immiscible"] = dict(E=eng.mixture_energy()["E"], E_sym=E_sym, E_sep=E_sep, g=a.g, g12=a.g12_immiscible, mu1=m["mu1"], mu2=m["mu2"], integral1=m["integral1"], integral2=m["integral2"], loss=sc["loss"],
                         pde=sc["pde"], density_overlap=float(dx * np.sqrt(d1 * d2).sum() / np.sqrt(m["integral1"] * m["integral2"])),
                         centre_of_mass=[float((x[:, 0] * d).sum() / d.sum()) for d in (d1, d2)],
                         residual_rms=[float(np.sqrt(dx * (r[:, k] ** 2).sum())) for k in range(2)], train_seconds=secs)
eng.close()
txt = json.dumps(rec, indent=1)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(txt + "\n")
