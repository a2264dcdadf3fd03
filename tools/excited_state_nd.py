#!/usr/bin/env python3
"""First excited state in 2D on sampler-drawn collocation sets, by deflation against a FROZEN ground state
(Engine.bind_orth_state): what gpe_bind_orth alone could not do, because a caller's psi_0 array lives on fixed points.

  1. ground state: [2, 64 x 4, 1], gamma = 0, pre-trained on the analytic Gaussian (the reference's own strategy, as
     tools/accuracy_nd.py), then trained with the device sampler and the variational energy term;
  2. frozen with amplitude = 1 / sqrt(observables()["norm"]) into slot 0 of a second engine (fresh parameters, no pre-training),
     which trains with w_orth > 0 on its own sampler: the energy minimiser in the orthogonal complement is the first excited state.
At gamma = 0 the exact eigenvalues are 2 sqrt(c pot_scale) (n_x + n_y + 1): 1 and 2 for c = pot_scale = 1/2, omega = 1.

--timing: ms/step of [2, 64 x 4, 1] with and without one frozen state at 1 048 576 points (every = 100 and 1) and 4 096 points
(every = 1).  The state's cost has two parts: the orthogonality term in the step itself (head and seed kernels, no head fusion)
and one value-only forward pass + k_orth_fill per redraw.

One JSON object (--out, default bench_out/excited_state_2d.json); no pass bar."""
import argparse, json, math, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import gpe_pinn
from gpe_pinn import capi
from gpe_pinn.sampler import node_centred
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=128, help="grid cells per axis")
ap.add_argument("--half", type=float, default=6.0)
ap.add_argument("--pretrain", type=int, default=2000)
ap.add_argument("--epochs", type=int, default=40000, help="steps per state")
ap.add_argument("--every", type=int, default=10, help="steps between redraws of the collocation set")
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--w-orth", type=float, default=100.0)
ap.add_argument("--w-norm", type=float, default=100.0)
ap.add_argument("--w-riesz", type=float, default=1.0)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--keep-best", action="store_true", help="ground state: a keeper (Engine.bind_keeper) on a monitor of the regular grid keeps the parameters of the "
                "lowest res_rms, and psi_0 is frozen from THEM (which=\"best\") instead of from the last step")
ap.add_argument("--timing", action="store_true", help="also measure ms/step with and without one frozen state")
ap.add_argument("--timing-only", action="store_true")
ap.add_argument("--steps", type=int, default=300, help="--timing: steps per timed pass")
ap.add_argument("--out", default="")
a = ap.parse_args()

LAYERS = [2, 64, 64, 64, 64, 1]
n, half = a.n, a.half
ax = np.linspace(-half, half, n)
h = ax[1] - ax[0]
dv = float(h * h)
X = np.stack([m.ravel() for m in np.meshgrid(ax, ax, indexing="ij")], axis=1).astype(np.float32)
t = np.linspace(-half, half, 64, endpoint=False)
xb = np.concatenate([np.stack(c, axis=1) for c in ((np.full(64, -half), t), (np.full(64, half), t), (t, np.full(64, -half)), (t, np.full(64, half)))]).astype(np.float32)
S_LO, S_HI, S_CLIP = node_centred([half, half], [n, n])


def make(seed, w_orth):
    cfg = gpe_pinn.GPEConfig(layers=LAYERS, gamma=0.0, p=3, kinetic_coeff=0.5, pot_scale=0.5, dx=dv, w_bc=10.0, w_norm=a.w_norm, w_orth=w_orth,
                             lr=a.lr, sched=capi.SCHED_CONST, history_capacity=8, w_riesz=a.w_riesz, riesz_kind=capi.RIESZ_VARIATIONAL)
    eng = gpe_pinn.Engine(cfg)
    eng.set_params(bench.reference_init(LAYERS, seed=seed))
    eng.bind_points(torch.as_tensor(X, device="cuda"))
    eng.bind_boundary(torch.as_tensor(xb, device="cuda"))
    return eng


def train(eng, tag, t0, keep_best=False):
    """--epochs steps on the device sampler, learning rate stepped down (Adam state kept); the numbers on the REGULAR grid.
    keep_best: the regular grid as held-out monitor every 10 redraws, and a keeper on its res_rms"""
    eng.bind_sampler(S_LO, S_HI, (n, n), every=a.every, seed=1234 + a.seed, clip=S_CLIP)
    eng.reset_optimizer(a.lr)
    if keep_best:
        eng.bind_monitor(torch.as_tensor(X, device="cuda"), every=10 * a.every, dv=dv)
        eng.bind_keeper("res_rms")
    for frac, lr in ((0.5, a.lr), (0.2, a.lr * 0.3), (0.15, a.lr * 0.1), (0.1, a.lr * 0.03), (0.05, a.lr * 0.01)):
        eng.set_lr(lr)
        eng.run(int(a.epochs * frac))
        sc = eng.read_scalars()
        print(f"   {tag}: lr {lr:.1e} mu {sc['mu']:.6f} pde {sc['pde']:.3e} int {sc['integral']:.6f} orth {sc['orth']:.3e} ({time.time() - t0:.0f} s)", flush=True)
    eng.bind_points(torch.as_tensor(X, device="cuda"))
    sc = eng.residual(want_fields=False)[0]
    ob = eng.observables()
    return sc, ob


out = dict(layers=LAYERS, gamma=0.0, kinetic_coeff=0.5, pot_scale=0.5, omega=1.0, exact_mu=[1.0, 2.0], grid_per_axis=n, half=half, points=int(X.shape[0]),
           schedule=dict(pretrain_ground=a.pretrain, pretrain_excited=0, epochs_per_state=a.epochs, every=a.every, lr=a.lr, w_orth=a.w_orth, w_norm=a.w_norm,
                         w_riesz=a.w_riesz, sampler="device", lr_ladder="lr x (1, 0.3, 0.1, 0.03, 0.01) over (0.5, 0.2, 0.15, 0.1, 0.05) of the steps"))

if not a.timing_only:
    t0 = time.time()
    g = make(a.seed, 0.0)
    phi0 = (1.0 / math.pi) ** 0.5 * np.exp(-0.5 * (X.astype(np.float64) ** 2).sum(axis=1))
    g.bind_target(torch.as_tensor(phi0.astype(np.float32), device="cuda"))
    g.reset_optimizer(a.lr)
    for i in range(a.pretrain):
        g.lib.gpe_mse_begin(g._h); g.lib.gpe_mse_update(g._h)
    g.bind_target(None)
    sc0, ob0 = train(g, "ground", t0, keep_best=a.keep_best)
    which = "last"
    if a.keep_best:                          # the numbers of the kept set replace those of the last step: psi_0 is frozen from it
        rec, ks = g.best_record(), g.keeper_state()
        print(f"ground state, last step: mu {ob0['mu']:.6f}  res_rms {ob0['res_rms']:.3e};  kept (step {rec['step']:.0f}, {ks['kept']} of {ks['seen']} records "
              f"improved): mu {rec['mu']:.6f}  res_rms {rec['res_rms']:.3e}", flush=True)
        out.update(ground_last=dict(mu=ob0["mu"], res_rms=ob0["res_rms"]), ground_kept_step=rec["step"])
        ob0, which = rec, "best"
    t_ground = time.time() - t0
    print(f"ground state: mu {ob0['mu']:.6f} (exact 1)  E {ob0['energy']:.6f}  norm {ob0['norm']:.6f}  res_rms {ob0['res_rms']:.3e}  ({t_ground:.0f} s)", flush=True)

    t1 = time.time()
    x = make(a.seed + 1, a.w_orth)
    x.bind_orth_state(0, g, amplitude=1.0 / math.sqrt(ob0["norm"]), which=which)
    sc1, ob1 = train(x, "excited", t1)
    t_excited = time.time() - t1
    psi0 = x.orth_values(0).double()                                   # the frozen, normalised ground state on the regular grid
    u = x.residual()[1][:, 0].double()
    overlap_raw = float(dv * (psi0 * u).sum())
    overlap = overlap_raw / math.sqrt(ob1["norm"])
    print(f"excited state: mu {ob1['mu']:.6f} (exact 2)  E {ob1['energy']:.6f}  norm {ob1['norm']:.6f}  overlap with psi_0 {overlap:.3e}  "
          f"res_rms {ob1['res_rms']:.3e}  ({t_excited:.0f} s)", flush=True)
    keys = ("norm", "kin", "pot", "inter", "energy", "mu", "mu_lap", "mean_x", "var_x", "peak_density", "res_rms")
    out.update(ground=dict(mu=ob0["mu"], mu_abs_err=abs(ob0["mu"] - 1.0), rayleigh_mu=sc0["mu"], seconds=t_ground, observables={k: ob0[k] for k in keys}),
               excited=dict(mu=ob1["mu"], mu_abs_err=abs(ob1["mu"] - 2.0), rayleigh_mu=sc1["mu"], seconds=t_excited, orth_term=sc1["orth"],
                            overlap_dv_sum_psi0_u=overlap_raw, overlap_normalised=overlap, psi0_norm_on_grid=float(dv * (psi0 * psi0).sum()),
                            observables={k: ob1[k] for k in keys}),
               seconds=time.time() - t0)
    g.close(); x.close()

if a.timing or a.timing_only:
    rows = []
    for side, every in ((1024, 100), (1024, 1), (64, 1)):
        lo, hi, clip = node_centred([8.0, 8.0], [side, side])
        res = {}
        for with_state in (False, True):
            cfg = gpe_pinn.GPEConfig(layers=LAYERS, gamma=500.0, dx=float((16.0 / (side - 1)) ** 2), w_bc=0.0, w_orth=1.0 if with_state else 0.0,
                                     sched=capi.SCHED_CONST, history_capacity=8)
            eng = gpe_pinn.Engine(cfg)
            eng.set_params(bench.reference_init(LAYERS))
            if with_state:
                eng.bind_orth_state(0, bench.reference_init(LAYERS, seed=7))
            eng.bind_sampler(lo, hi, (side, side), every=every, seed=1, clip=clip)
            eng.run(max(a.steps // 4, 2 * every if every < 50 else 50))
            eng.synchronize()
            times = []
            for _ in range(3):
                tt = time.perf_counter()
                eng.run(a.steps)
                eng.synchronize()
                times.append((time.perf_counter() - tt) / a.steps * 1e3)
            res[with_state] = float(np.median(times))
            rows.append(dict(points=side * side, every=every, frozen_states=int(with_state), steps=a.steps, ms_per_step_median=res[with_state], ms_per_step_passes=times))
            print(json.dumps(rows[-1]), flush=True)
            eng.close()
            torch.cuda.empty_cache()
        rows.append(dict(points=side * side, every=every, added_ms_per_step=res[True] - res[False], added_pct=(res[True] / res[False] - 1) * 100))
        print(json.dumps(rows[-1]), flush=True)
    out["step_time"] = rows

path = a.out or os.path.join(ROOT, "bench_out", "excited_state_2d.json")
os.makedirs(os.path.dirname(path), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print("wrote", path)
