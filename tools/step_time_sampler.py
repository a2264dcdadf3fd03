#!/usr/bin/env python3
"""Wall time per step of gpe_run under a device-side sampler that redraws every 100 steps, NS network (harmonic trap, north-star loss):
    step_time_sampler.py graded N_PER_AXIS [steps] [blocks]          graded sampler, N_PER_AXIS^2 cells (sinh_edges, stretch 2)
    step_time_sampler.py adaptive N_PER_AXIS [steps] [blocks]        adaptive sampler, N_PER_AXIS^2 rows on 32 x 32 blocks (same stretch)
    step_time_sampler.py residual N_PER_AXIS                         one gpe_residual on the graded set: the launches the adaptive detour makes
    step_time_sampler.py uniform N_PER_AXIS [steps] [blocks] [every] plain sampler, N_PER_AXIS^2 cells of the uniform grid (dx = the cell volume)
    step_time_sampler.py cells N_PER_AXIS [steps] [blocks] [every]   cell-subset sampler on the FULL list of that grid: the same rows and step
                                                                     kernels as `uniform`, so the two differ by the indirection of the redraw alone
    step_time_sampler.py disk N_PER_AXIS [steps] [blocks] [every]    cell-subset sampler on the inscribed disk (0.785 of the rows)
Best of `blocks` timed blocks of `steps` steps (a multiple of 100, so every block holds the same number of redraws)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import gpe_pinn
from gpe_pinn.sampler import sinh_edges

mode, n = sys.argv[1], int(sys.argv[2])
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 400
blocks = int(sys.argv[4]) if len(sys.argv) > 4 else 5
EVERY, HALF, LAYERS = (int(sys.argv[5]) if len(sys.argv) > 5 else 100), 6.0, [2, 64, 64, 64, 64, 1]
UNWEIGHTED = mode in ("uniform", "cells", "disk")
cfg = gpe_pinn.GPEConfig(layers=LAYERS, gamma=100.0, dx=(2.0 * HALF / n) ** 2 if UNWEIGHTED else 1.0, lr=1e-3, w_bc=0.0)
eng = gpe_pinn.Engine(cfg)
torch.manual_seed(0)
eng.set_params((torch.randn(len(eng.get_params())) * 0.1).numpy())
if mode == "adaptive":
    eng.bind_sampler_adaptive([sinh_edges(HALF, 32, 2.0)] * 2, n_points=n * n, every=EVERY, seed=7, n_min=1, uniform_share=0.5)
elif mode == "uniform":
    eng.bind_sampler((-HALF,) * 2, (HALF,) * 2, (n, n), every=EVERY, seed=7)
elif mode in ("cells", "disk"):
    from gpe_pinn.sampler import ball_cells
    cells = np.arange(n * n, dtype=np.int64) if mode == "cells" else ball_cells((-HALF,) * 2, (HALF,) * 2, (n, n), HALF)
    eng.bind_sampler_cells(cells, (-HALF,) * 2, (HALF,) * 2, (n, n), every=EVERY, seed=7)
else:
    eng.bind_sampler_graded([sinh_edges(HALF, n, 2.0)] * 2, every=EVERY, seed=7)
eng.run(2 * EVERY); eng.synchronize()
if mode == "residual":
    t = []
    for _ in range(20):
        t0 = time.perf_counter(); eng.residual(want_fields=False); t.append((time.perf_counter() - t0) * 1e6)
    print("residual N=%d: %.1f us per call (best of 20, with its synchronisation and read-back); / %d = %.2f us per step" % (n * n, min(t), EVERY, min(t) / EVERY))
    sys.exit(0)
t = []
for _ in range(blocks):
    t0 = time.perf_counter(); eng.run(steps); eng.synchronize(); t.append((time.perf_counter() - t0) / steps * 1e6)
print("%s N=%d every=%d: %.2f us/step best of %d x %d steps (all: %s)" % (mode, eng.n_local, EVERY, min(t), blocks, steps, " ".join("%.2f" % v for v in t)))
