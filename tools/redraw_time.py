#!/usr/bin/env python3
"""HIP-event time of a sampler's redraw launch, NS network (2,64,64,64,64,1), by difference on the engine's own stream:
    redraw_time.py {uniform|cells|terms} N_PER_AXIS [steps] [blocks]
Two engines on the same grid and seed, one with every = 1 (a redraw is enqueued before every step) and one that never redraws; blocks of
`steps` steps of gpe_run are bracketed by a pair of events on the stream the engine enqueues on (torch's current stream), the two engines
alternating, and the best block of each is kept.  (every = 1) - (no redraw), per step, is what one redraw adds to the stream: the kernel
and its launch, as the step sees them.  uniform = gpe_bind_sampler; cells = gpe_sampler_cells on the full list of the same grid;
terms = gpe_bind_sampler on an engine whose potential is a 4-term table (gpe_potential_terms: the redraw is the draw kernel plus the fill
of the engine-owned V; both engines run the step on the precomputed-potential path)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import gpe_pinn

mode, n = sys.argv[1], int(sys.argv[2])
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
blocks = int(sys.argv[4]) if len(sys.argv) > 4 else 7
HALF, LAYERS = 6.0, [2, 64, 64, 64, 64, 1]


def engine(every):
    kw = dict(potential=gpe_pinn.POT_PRECOMPUTED) if mode == "terms" else {}
    eng = gpe_pinn.Engine(gpe_pinn.GPEConfig(layers=LAYERS, gamma=100.0, dx=(2.0 * HALF / n) ** 2, lr=1e-3, w_bc=0.0, **kw))
    if mode == "terms":
        P = gpe_pinn.potential
        eng.bind_potential_terms([P.quadratic(0.5, (1.0, 1.4), (0.3, -0.2)), P.gaussian(-2.0, (1.2, 1.2), (-0.5, 0.4)), P.quartic(0.01, (1.0, 1.0)),
                                  P.lattice(1.5, (2.0, 0.0))])
    torch.manual_seed(0)
    eng.set_params((torch.randn(len(eng.get_params())) * 0.1).numpy())
    g = dict(lo=(-HALF,) * 2, hi=(HALF,) * 2, shape=(n, n), every=every, seed=7)
    if mode == "cells":
        eng.bind_sampler_cells(np.arange(n * n, dtype=np.int64), **g)
    else:
        eng.bind_sampler(**g)
    eng.run(steps); eng.synchronize()
    return eng


def block(eng):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); eng.run(steps); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


with_redraw, without = engine(1), engine(1 << 40)
t1, t0 = [], []
for _ in range(blocks):
    t1.append(block(with_redraw)); t0.append(block(without))
print("%s N=%d: redraw %.2f us by HIP events (every = 1: %.2f us/step, no redraw: %.2f us/step; best of %d x %d steps; all differences: %s)"
      % (mode, n * n, min(t1) - min(t0), min(t1), min(t0), blocks, steps, " ".join("%.2f" % (p - q) for p, q in zip(t1, t0))))
