"""The cells of tests/test_gpu_observe_instances.py and tools/observe_record_bits.py: one per instance of the observables chain (2 kinds x
3 dims x weighted or not) and size, each on an engine with a PRECOMPUTED fp32 potential, so that host sums over the engine's own jets
take the very numbers the kernels read.  Fixed seeds; nothing here needs a GPU until a cell is run."""
import numpy as np

from gpe_pinn import Engine, capi
from oracle import gpe_oracle as go
from tests import mixture_cases as mc
from tests.test_gpu_mixture import config, dev
from tests.test_gpu_parity import _inputs, cfg_from_problem

SIZES = (1, 257, 262149)      # one thread; one workgroup and one point; OBS_MAX_WG * OBS_THREADS + 5: threads loop
SCALAR = {"real_1d": (1, False), "real_2d": (2, False), "real_3d": (3, False), "complex_rot_2d": (2, True), "complex_rot_3d": (3, True)}


def weights(N):
    return np.random.default_rng(N + 3).uniform(0.5, 1.5, N).astype(np.float32)


def _run(eng, x, V, dv, weighted, observe):
    """-> (own jets in fp64, weights or None, the record): no weights on an explicit set, real positive weights on the bound set"""
    try:
        J = eng.forward_jets(dev(x)).cpu().numpy().astype(np.float64)
        if not weighted:
            return J, None, observe(eng)(dev(x), V=dev(V), dv=dv)
        q = weights(x.shape[0])
        eng.bind_points(dev(x), V=dev(V))
        eng.bind_weights(dev(q))
        return J, q.astype(np.float64), observe(eng)(dv=dv)
    finally:
        eng.close()


def scalar_cell(name, N, weighted):
    """-> (Problem, x, V, dv, J, q, record)"""
    d, cplx = SCALAR[name]
    kw = dict(layers=[d, 32, 32, 2 if cplx else 1], gamma=30.0 if cplx else 20.0, dx=0.02 if cplx else 0.01, potential=go.POT_PRECOMPUTED)
    if cplx:
        kw.update(complex_psi=True, omega_rot=0.8)
    x, flat, _ = _inputs(kw, N)
    V = np.random.default_rng(d + 11).uniform(0.0, 3.0, N).astype(np.float32)
    pb = go.Problem(**kw)
    cfg = cfg_from_problem(pb)
    cfg.w_bc = 0.0
    eng = Engine(cfg)
    eng.set_params(flat)
    return (pb, x, V, pb.dx) + _run(eng, x, V, pb.dx, weighted, lambda e: e.observables)


def mixture_cell(d, N, weighted):
    """-> (MixProblem, x, V, dv, J, q, record)"""
    layers = [d, 32, 32, 32, 2]
    x, flat, _, _ = mc.inputs(layers, N, seed=d)
    V = np.random.default_rng(d + 1).uniform(0.0, 3.0, N).astype(np.float32)
    mp = mc.problem(layers, N, potential=capi.POT_PRECOMPUTED)
    dv = 4.0 ** d / N
    eng = Engine(config(mp))
    eng.set_params(flat)
    return (mp, x, V, dv) + _run(eng, x, V, dv, weighted, lambda e: e.mixture_observables)
