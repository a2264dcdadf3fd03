#!/usr/bin/env python3
"""Wall time per step of gpe_run for any network / batch size (harmonic trap, north-star loss):  step_time_nd.py 2,128,128,128,128,128,1 16384 [steps] [ones]
A fourth argument `ones` binds quadrature weights of 1 (Engine.bind_weights): the same step on the standalone weighted head / seed kernels.
`terms`: the potential is a 4-term table (Engine.bind_potential_terms) and the engine fills V itself; `array`: the same V handed over as a
caller's array on the same precomputed-potential path (the two are expected to step equally fast: the kernels are the same)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import gpe_pinn
layers = [int(v) for v in sys.argv[1].split(",")]
N = int(sys.argv[2]); steps = int(sys.argv[3]) if len(sys.argv) > 3 else 400
d = layers[0]
rng = np.random.default_rng(0)
x = rng.uniform(-6, 6, (N, d)).astype(np.float32)
opt = sys.argv[4] if len(sys.argv) > 4 else ""
pre = opt in ("terms", "array")
cfg = gpe_pinn.GPEConfig(layers=layers, gamma=100.0, dx=float(12.0 ** d / N), lr=1e-3, complex_psi=layers[-1] == 2,
                         **(dict(potential=gpe_pinn.POT_PRECOMPUTED) if pre else {}))
eng = gpe_pinn.Engine(cfg)
torch.manual_seed(0)
eng.set_params((torch.randn(eng.n_params) * 0.1).numpy())
if pre:
    P = gpe_pinn.potential
    table = [P.quadratic(0.5, (1.0, 1.4, 0.8)[:d], (0.3, -0.2, 0.1)[:d]), P.gaussian(-2.0, (1.2,) * d, (-0.5, 0.4, 0.0)[:d]), P.quartic(0.01, (1.0,) * d),
             P.lattice(1.5, (2.0,) + (0.0,) * (d - 1))]
    eng.bind_potential_terms(table)
    if opt == "terms":
        eng.bind_points(torch.as_tensor(x, device="cuda"))
    else:                                                 # the same values as a caller's array, on an engine without terms
        V = eng.potential_at(x)
        eng.clear_potential_terms()
        eng.bind_points(torch.as_tensor(x, device="cuda"), V=V)
else:
    eng.bind_points(torch.as_tensor(x, device="cuda"))
ones = opt == "ones"
if ones:
    eng.bind_weights(torch.ones(N, device="cuda"))
eng.run(30); eng.synchronize()
t = []
for _ in range(3):
    t0 = time.perf_counter(); eng.run(steps); eng.synchronize(); t.append((time.perf_counter() - t0) / steps * 1e6)
k = eng.active_kernels
print("%s N=%d%s: %.1f us/step  %.3g points/s  fwd=%s bwd=%s" % (sys.argv[1], N, " weights=1" if ones else (" potential=" + opt if pre else ""), min(t), N / min(t) * 1e6, k["fwd"][:28], k["bwd"][:28]))
