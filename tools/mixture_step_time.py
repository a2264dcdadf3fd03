#!/usr/bin/env python3
"""Step time of a two-component mixture against the complex-psi step of the same shape ([2,64,64,64,2], 65 536 points by default): both
run the same n_out = 2 forward / reverse kernels, the difference is the standalone head / seed pair (k_head_mix / k_seed_mix against
k_head_pde / k_seed_pde).  Medians of --blocks timed blocks of --steps steps each (gpe_run, HIP events), after a warm-up block; the
engines alternate block by block.  --energy W adds a third engine: the mixture with its energy term on (gpe_mixture_energy_weight: the
energy instances of the head / seed pair), against the plain mixture step.
usage: tools/mixture_step_time.py [--points N] [--energy W] > profiles/mixture/step_time.txt"""
import argparse, os, statistics, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpe_pinn
from bench import reference_init

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=65536)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--blocks", type=int, default=21)
ap.add_argument("--energy", type=float, default=0.0, help="also time the mixture step with the energy term at this weight")
a = ap.parse_args()
layers, N = [2, 64, 64, 64, 2], a.points
rng = np.random.default_rng(0)
x = torch.as_tensor((rng.random((N, 2)) * 8 - 4).astype(np.float32), device="cuda")
xb = torch.as_tensor((rng.random((64, 2)) * 8 - 4).astype(np.float32), device="cuda")
common = dict(layers=layers, kinetic_coeff=0.5, pot_scale=0.5, dx=64.0 / N, w_bc=10.0, w_norm=20.0, lr=1e-4, n_global=N)
engs = {"complex_psi": gpe_pinn.Engine(gpe_pinn.GPEConfig(complex_psi=True, gamma=10.0, **common)),
        "mixture": gpe_pinn.Engine(gpe_pinn.GPEConfig(mixture=True, mix_g=(10.0, 8.0, 6.0), mix_norm=(0.5, 0.5), **common))}
if a.energy > 0:
    engs["mixture_energy"] = gpe_pinn.Engine(gpe_pinn.GPEConfig(mixture=True, mix_g=(10.0, 8.0, 6.0), mix_norm=(0.5, 0.5), **common))
    engs["mixture_energy"].set_mixture_energy(a.energy)
for e in engs.values():
    e.set_params(reference_init(layers, seed=1))
    e.bind_points(x); e.bind_boundary(xb)
    e.run(a.steps); e.synchronize()
ms = {k: [] for k in engs}
for _ in range(a.blocks):
    for k, e in engs.items():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); e.run(a.steps); t1.record(); e.synchronize()
        ms[k].append(t0.elapsed_time(t1) / a.steps)
for k, e in engs.items():
    v = sorted(ms[k])
    print(f"{k:12s} {layers} N={N}: median {statistics.median(v) * 1e3:8.1f} us/step  (min {v[0] * 1e3:.1f}, max {v[-1] * 1e3:.1f}, {a.blocks} blocks of {a.steps})  "
          f"{e.active_kernels}", flush=True)
m, c = statistics.median(ms["mixture"]), statistics.median(ms["complex_psi"])
print(f"mixture - complex_psi: {(m - c) * 1e3:+.1f} us/step ({(m / c - 1) * 100:+.2f} %)")
if a.energy > 0:
    t = statistics.median(ms["mixture_energy"])
    print(f"mixture_energy - mixture: {(t - m) * 1e3:+.1f} us/step ({(t / m - 1) * 100:+.2f} %)")
