"""The mixture cases tests/test_gpu_mixture.py steps on the GPU, and their inputs.  tests/test_mixture_reference_cpu.py asserts on these
very inputs that a gradient without the cross term of the seeds is off by percents -- so a kernel that forgot the term cannot pass.

Couplings g11 != g22, g12 != 0 and norms n_1 != n_2 throughout.  Six boundary rows with a target per case; the engine merges them into
the collocation launch when 6 * 8 <= N (N = 49, 300, 1 025) and runs them as a batch of their own below that (N = 37)."""
import numpy as np

from oracle import gpe_oracle as go
from tests import mixture_ref as mr

G = (6.0, 3.0, 8.0)
NORMS = (0.6, 0.4)
N_BC = 6

# name: (layers, N, path ("fused" / "generic"), activation)
CASES = {
    "fused_2d_64x3_N37": ([2, 64, 64, 64, 2], 37, "fused", 0),
    "fused_2d_64x3_N49": ([2, 64, 64, 64, 2], 49, "fused", 0),
    "fused_2d_64x3_N1025": ([2, 64, 64, 64, 2], 1025, "fused", 0),
    "fused_2d_32x3_N37": ([2, 32, 32, 32, 2], 37, "fused", 1),
    "fused_2d_32x3_N1025": ([2, 32, 32, 32, 2], 1025, "fused", 1),
    "fused_2d_128x2_N37": ([2, 128, 128, 2], 37, "fused", 0),
    "fused_2d_128x2_N1025": ([2, 128, 128, 2], 1025, "fused", 0),
    "padded_2d_72x3_N37": ([2, 72, 72, 72, 2], 37, "fused", 0),
    "padded_2d_72x3_N1025": ([2, 72, 72, 72, 2], 1025, "fused", 1),
    "wide_3d_256x2_N300": ([3, 256, 256, 2], 300, "fused", 0),
    "generic_1d_48x2_N37": ([1, 48, 48, 2], 37, "generic", 1),
    "generic_1d_48x2_N1025": ([1, 48, 48, 2], 1025, "generic", 0),
    "generic_2d_64x2_N37": ([2, 64, 64, 2], 37, "generic", 0),
    "generic_2d_64x2_N1025": ([2, 64, 64, 2], 1025, "generic", 1),
    "generic_3d_40_N37": ([3, 40, 2], 37, "generic", 0),
    "generic_3d_40_N1025": ([3, 40, 2], 1025, "generic", 0),
}


def weight_scale(layers):
    """~ 2.4 / sqrt(H), as tests/test_gpu_parity.py scales its networks: tanh stays out of saturation, every jet channel O(1)"""
    w = max(layers[1:-1])
    return 0.3 if w <= 64 else (0.15 if w <= 128 else 0.1)


def problem(layers, N, activation=0, g=G, norms=NORMS, **kw):
    d = dict(layers=list(layers), activation=activation, kinetic_coeff=0.5, potential=go.POT_HARMONIC, pot_scale=0.5, gamma=0.0, p=3,
             perturb_scale=1.0, bc_nn_scale=1.0, w_pde=1.0, w_bc=10.0, w_norm=20.0, dx=1.0 / N)
    d.update(kw)
    return mr.MixProblem(go.Problem(**d), tuple(g), tuple(norms))


def inputs(layers, N, seed=0):
    """(x [N, d], flat, x_bc [6, d], bc_target [6, 2]) in float32"""
    rng = np.random.default_rng(seed)
    d = layers[0]
    x = np.linspace(-3, 3, N).reshape(-1, 1) if d == 1 else rng.uniform(-2, 2, (N, d))
    flat = rng.normal(0, 1, go.param_count(layers)) * weight_scale(layers)
    x_bc = rng.uniform(-3, 3, (N_BC, d))
    tgt = rng.normal(0, 0.1, (N_BC, 2))
    return x.astype(np.float32), flat.astype(np.float32), x_bc.astype(np.float32), tgt.astype(np.float32)


def case(name):
    """-> (MixProblem, x, flat, x_bc, bc_target, path)"""
    layers, N, path, act = CASES[name]
    return (problem(layers, N, act),) + inputs(layers, N) + (path,)
