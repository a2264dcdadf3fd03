#!/usr/bin/env python3
"""Time of one Engine.observables() call on the bound set (forward of the full jets, the four-launch chain, one record to the host), at
the grids of tools/keeper_time.py: 3 969, 16 384 and 1 048 576 points of [2,64,64,64,64,1].  Host clock around 50 synchronising calls,
median / min / max of --reps repeats.  Compare two library builds with GPE_HIP_LIB=... on one box, alternating.

usage: python tools/observables_call_time.py [--reps 9]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench, gpe_pinn
from gpe_pinn import capi

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
a = ap.parse_args()
layers = [2, 64, 64, 64, 64, 1]
for n in (3969, 16384, 1 << 20):
    k = int(round(n ** 0.5))
    ax = np.linspace(-8, 8, k, dtype=np.float32)
    X = np.stack([m.ravel() for m in np.meshgrid(ax, ax, indexing="ij")], axis=1)
    eng = gpe_pinn.Engine(gpe_pinn.GPEConfig(layers=layers, gamma=500.0, dx=float(ax[1] - ax[0]) ** 2, w_bc=0.0, lr=1e-4, sched=capi.SCHED_CONST))
    eng.set_params(bench.reference_init(layers, seed=0))
    eng.bind_points(torch.as_tensor(X, device="cuda"))
    for _ in range(20):
        eng.observables()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(50):
            eng.observables()
        ts.append((time.perf_counter() - t0) / 50 * 1e6)
    print(f"observables() on the bound set, {X.shape[0]} points: median {np.median(ts):.1f} us/call, min {min(ts):.1f}, max {max(ts):.1f} "
          f"({a.reps} x 50 calls)", flush=True)
    eng.close()
