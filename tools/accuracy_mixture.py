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
The final numbers of a state (mu_a, norms, energy, overlap, centres, residuals) come from the device: gpe_mixture_observables on the
evaluation grid (twice as fine as the training grid); the host sums over the residual fields on the training grid are kept as a printed
cross-check.  --monitor EVERY --keeper METRIC train with that grid as a held-out monitor (gpe_mixture_monitor) and the keeper
(gpe_mixture_keeper) on METRIC through the last continuation stage, and report the kept state next to the last one.
usage: tools/accuracy_mixture.py [--energy W] [--monitor EVERY --keeper res_rms|energy] [--out profiles/mixture_observe/accuracy_mixture_1d.json]"""
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
ap.add_argument("--monitor", type=int, default=0, help="held-out monitor on the evaluation grid every EVERY steps of the last stage (0: none)")
ap.add_argument("--keeper", choices=["res_rms", "energy"], default=None, help="keep the best parameters by this field of the monitor's records")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if a.keeper and a.monitor <= 0:
    ap.error("--keeper needs --monitor EVERY")

layers, N, L = [1, 64, 64, 64, 2], a.points, a.half
x = np.linspace(-L, L, N, dtype=np.float64).reshape(-1, 1)
dx = 2 * L / (N - 1)
xd = torch.as_tensor(x.astype(np.float32), device="cuda")
xb = torch.as_tensor(np.array([[-L], [L]], np.float32), device="cuda")
xe = torch.linspace(-L, L, 2 * N - 1, device="cuda").reshape(-1, 1)          # evaluation grid: observables, monitor
dxe = 2 * L / (2 * N - 2)


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
            if a.monitor > 0:                    # the metric is comparable at fixed couplings only: watch the last stage
                eng.bind_mixture_monitor(xe, every=a.monitor, dv=dxe)
                if a.keeper:
                    eng.bind_mixture_keeper(a.keeper)
        eng.run(a.steps)
    eng.synchronize()
    return eng, time.time() - t0


def state(eng):
    sc, psi, res = eng.residual()
    return sc, eng.mixture_scalars(), psi.cpu().numpy().astype(np.float64), res.cpu().numpy().astype(np.float64)


def device_numbers(eng, m, r):
    """the state's numbers from gpe_mixture_observables on the evaluation grid; the host sums on the training grid printed beside them"""
    o = eng.mixture_observables(xe, dv=dxe)
    host_rms = [float(np.sqrt(dx * (r[:, k] ** 2).sum())) for k in range(2)]
    print(f"[cross-check] device mu {o['mu']} (step record, training grid: {m['mu1']}, {m['mu2']});  device norm {o['norm']} (host "
          f"{m['integral1']}, {m['integral2']});  device res_rms of the normalised state {o['res_rms']} (host, raw state: {host_rms})", file=sys.stderr)
    return o


def kept_and_last(eng, m, r):
    """dict(last=..., kept=..., keeper=...) with a keeper; the last state's numbers alone without"""
    out = dict(last=device_numbers(eng, m, r))
    if a.monitor > 0:
        recs = eng.read_mixture_monitor()
        out["monitor"] = dict(every=a.monitor, records=len(recs), **{k: [rec[k] for rec in recs] for k in ("step", "energy", "res_rms_total", "overlap")})
    if a.keeper:
        out["keeper"] = dict(metric=a.keeper, **eng.keeper_state())
        out["kept"] = eng.best_record()
        eng.restore_best()
        out["kept_reevaluated"] = eng.mixture_observables(xe, dv=dxe)
    return out


rec = dict(tool="tools/accuracy_mixture.py", energy_weight=a.energy, monitor_every=a.monitor, keeper=a.keeper, evaluation_points=2 * N - 1, layers=layers, points=N, box=[-L, L], dx=dx, stages=a.stages, steps_per_stage=a.steps, pretrain=a.pretrain)
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
sym["observables"] = kept_and_last(eng, m, r)
sym["mu_abs_err_device"] = [abs(v - lam[g_eff]) for v in sym["observables"]["last"]["mu"]]
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
rec["immiscible"]["observables"] = kept_and_last(eng, m, r)
eng.close()
txt = json.dumps(rec, indent=1)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(txt + "\n")
