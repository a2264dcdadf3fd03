#!/usr/bin/env python3
"""Time of one observables record (forward jets, reduction chain, copy back; the call synchronises) at 65 536 and 1 048 576 2D points:
gpe_mixture_observables beside gpe_observables of a real and of a complex-psi engine of the same network, and the forward pass alone.
usage: tools/mixture_observe_time.py > profiles/mixture_observe/record_time.txt"""
import sys, time, os
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpe_pinn
from bench import reference_init

def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)      # the call synchronises itself
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t))

for N in (65536, 1048576):
    x = torch.as_tensor((np.random.default_rng(0).random((N, 2)) * 8 - 4).astype(np.float32), device="cuda")
    dv = 64.0 / N
    for kind in ("scalar", "scalar_complex", "mixture"):
        out = 1 if kind == "scalar" else 2
        layers = [2, 64, 64, 64, out]
        kw = dict(layers=layers, kinetic_coeff=0.5, pot_scale=0.5, dx=dv)
        if kind == "scalar": kw.update(gamma=10.0)
        if kind == "scalar_complex": kw.update(gamma=10.0, complex_psi=True)
        if kind == "mixture": kw.update(mixture=True, mix_g=(6.0, 3.0, 8.0), mix_norm=(0.6, 0.4))
        eng = gpe_pinn.Engine(gpe_pinn.GPEConfig(**kw))
        eng.set_params(reference_init(layers, seed=1))
        call = (lambda: eng.mixture_observables(x, dv=dv)) if kind == "mixture" else (lambda: eng.observables(x, dv=dv))
        fwd = timed(lambda: (eng.forward_jets(x), None)[1])
        med, mn = timed(call)
        print(f"N {N:8d} {kind:15s} layers {layers}: one record (forward jets + chain + copy back) median {med:.3f} ms min {mn:.3f} ms;"
              f"  forward_jets alone median {fwd[0]:.3f} ms", flush=True)
        eng.close()
