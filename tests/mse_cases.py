"""The cases of the pre-training (MSE) step's oracle tests: networks, point counts, kernel sets, inputs, targets and the float64 /
float32 references.  Plain data and numpy: tests/test_mse_reference_cpu.py (no GPU) and tests/test_gpu_mse.py share it, and every
reference is computed once per process and left unchanged.

Inputs are those of test_step_matches_oracle (tests/test_gpu_parity.py: _inputs, _scale): weights N(0, 1) times 2.4 / sqrt(H)-ish,
x uniform in [-3, 3]^d (1D: linspace(-6, 6)); the box flavour has x = linspace(0, 1).  Targets leave every weight matrix and bias an
O(1) share of the gradient: exp(-|x|^2 / 2) (1 + 0.3 x_0), and for n_out = 2 a second channel x_1 exp(-|x|^2 / 4) (the imaginary part
of a vortex-like (x_0 + i x_1) exp(-|x|^2 / 4))."""
import numpy as np

from oracle import gpe_oracle as go
from tests import helpers as H
from tests.mse_ref import mse_loss_and_grad
from tests.test_gpu_parity import _inputs, _scale

RES = dict(net_kind=go.NET_RESIDUAL)

# name: (Problem kwargs, point counts, kernel sets, kernel family the cell reaches on the fused set)
SHAPES = {
    "1d_32x2": (dict(layers=[1, 32, 32, 1]), (1, 15, 16, 17, 333), ("fused", "generic"), "f_backward_pipe<32,1,0>"),
    "2d_64x4": (dict(layers=[2, 64, 64, 64, 64, 1]), (1, 15, 16, 17, 333), ("fused", "generic"), "f_backward_pipe<64,1,0>"),
    "3d_64x3": (dict(layers=[3, 64, 64, 64, 1]), (1, 15, 16, 17, 333), ("fused", "generic"), "f_backward_pipe<64,1,0> (the C = 5 exclusion of H = 64 in 3D does not apply at C = 1)"),
    # more tiles than the 2 * num_cu persistent workgroups; 32 785 points are above coop_fwd_max_tiles (8 tiles per CU), where the storing
    # per-wave f_forward<64,1,0> feeds the reverse pass
    "2d_64x4_large": (dict(layers=[2, 64, 64, 64, 64, 1]), (8209, 32785), ("fused",), "f_backward_pipe<64,1,0>, many tiles"),
    "2d_64x5_four_maps": (dict(layers=[2, 64, 64, 64, 64, 64, 1]), (401,), ("fused",), "f_backward_coop<64,1,0>, 4-5 maps"),
    "1d_64x6_five_maps": (dict(layers=[1, 64, 64, 64, 64, 64, 64, 1]), (401,), ("fused",), "f_backward_coop<64,1,0>, 4-5 maps"),
    "1d_res_64x2blocks": (dict(layers=[1, 64, 64, 64, 1], activation=1, **RES), (300,), ("fused", "generic"), "f_backward_coop<..,RES>"),
    "2d_res_32x2blocks": (dict(layers=[2, 32, 32, 32, 1], **RES), (300,), ("fused", "generic"), "f_backward_coop<..,RES>"),
    "2d_64x3_complex": (dict(layers=[2, 64, 64, 64, 2], complex_psi=True), (17, 600), ("fused",), "n_out = 2 at H = 64"),
    "2d_128x3": (dict(layers=[2, 128, 128, 128, 1]), (17, 300, 4113), ("fused",), "f_backward_coop<128,1,0>"),
    # at or above wide_min_tiles = 2 048 tiles: the wide set's per-map reverse kernels
    "2d_128x3_large": (dict(layers=[2, 128, 128, 128, 1]), (32785,), ("fused",), "w_bwd_map"),
    "2d_128x6_complex_cfg4": (dict(layers=[2, 128, 128, 128, 128, 128, 128, 2], complex_psi=True), (300,), ("fused",), "cfg4 network"),
    "2d_100x3_pads_to_128": (dict(layers=[2, 100, 100, 100, 1]), (300,), ("fused",), "padded widths"),
    "1d_20x3_pads_to_32": (dict(layers=[1, 20, 20, 20, 1]), (300,), ("fused",), "padded widths"),
    "2d_48_64_32_ragged": (dict(layers=[2, 48, 64, 32, 1]), (300,), ("fused",), "padded widths"),
    "3d_256x2": (dict(layers=[3, 256, 256, 1]), (300, 4099), ("fused", "generic"), "wide / generic set at H = 256"),
    "3d_256x6": (dict(layers=[3, 256, 256, 256, 256, 256, 256, 1]), (300, 4099), ("fused", "generic"), "wide / generic set at H = 256"),
    "1d_box_64x3": (dict(layers=[1, 64, 64, 64, 1], activation=1, base_kind=go.BASE_BOX, base_mode=0, envelope=go.ENV_SIN, env_L=1.0,
                         potential=go.POT_NONE, kinetic_coeff=1.0), (333,), ("fused",), "envelope factor"),
}

CELLS = [(name, N, path) for name, (_, ns, paths, _) in SHAPES.items() for N in ns for path in paths]


def target_of(x, n_out):
    x = np.asarray(x, np.float64)
    r2 = (x * x).sum(axis=1)
    t = np.exp(-0.5 * r2) * (1.0 + 0.3 * x[:, 0])
    if n_out == 1:
        return t[:, None]
    return np.stack([t, x[:, 1] * np.exp(-0.25 * r2)], axis=1)


_SETUP = {}


def setup(name, N):
    """problem, inputs (float32, what the engine is handed), target, parameter blocks and the references of (shape, N): loss / grad in
    float64, and the float32 run of the same reference as per-block and whole-vector errors against it"""
    key = (name, N)
    if key in _SETUP:
        return _SETUP[key]
    kw = SHAPES[name][0]
    pb = go.Problem(**kw)
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    if pb.envelope == go.ENV_SIN:
        x = np.linspace(0.0, 1.0, N, dtype=np.float32).reshape(-1, 1)
    target = target_of(x, pb.n_out).astype(np.float32)
    blocks = H.param_blocks(pb.layers, pb.net_kind)
    loss, grad = mse_loss_and_grad(pb, flat, x, target)
    loss32, grad32 = mse_loss_and_grad(pb, flat, x, target, dtype=np.float32)
    s = dict(pb=pb, kw=kw, N=N, x=x, flat=flat, x_bc=x_bc, target=target, blocks=blocks, loss=loss, grad=grad,
             f32_loss=abs(loss32 - loss) / loss, f32_whole=H.rel_err(grad32, grad), f32_blocks=H.block_rel_errs(grad32, grad, blocks))
    _SETUP[key] = s
    return s
