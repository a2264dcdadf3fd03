"""The pre-training (MSE) reference (tests/mse_ref.py) on any box: against torch.autograd in float64, and -- for every cell of
tests/test_gpu_mse.py -- its float32 run against its float64 run per parameter block, which is the condition that the inputs of the GPU
cells are well conditioned (every block below 1e-5 of its own maximum, so the 5e-5 asked of the engine has 5x to spare)."""
import math

import numpy as np
import pytest
import torch

from oracle import gpe_oracle as go
from oracle import torch_ref as tr
from tests import helpers as H
from tests import mse_cases as MC
from tests.mse_ref import mse_loss_and_grad

AUTOGRAD = {
    "mlp_tanh_2d": dict(layers=[2, 24, 24, 24, 1]),
    "shifted_tanh_1d": dict(layers=[1, 20, 20, 1], activation=1),
    "residual_2d": dict(layers=[2, 16, 16, 16, 1], net_kind=go.NET_RESIDUAL, activation=1),
    "complex_2d_two_outputs": dict(layers=[2, 24, 24, 2], complex_psi=True),
    "box_envelope_1d": dict(layers=[1, 20, 20, 1], activation=1, envelope=go.ENV_SIN, env_L=1.7, base_kind=go.BASE_BOX, base_mode=0),
}


@pytest.mark.parametrize("name", sorted(AUTOGRAD))
@pytest.mark.parametrize("n_global", [None, 100])
def test_reference_matches_autograd(name, n_global):
    kw = AUTOGRAD[name]
    pb = go.Problem(**kw)
    rng = np.random.default_rng(3)
    N, d = 37, pb.dim
    x = rng.uniform(0.0, 1.7, (N, d)) if pb.envelope == go.ENV_SIN else rng.uniform(-3, 3, (N, d))
    flat = rng.normal(0, 0.4, go.param_count(pb.layers, pb.net_kind))
    t = MC.target_of(x, pb.n_out)
    loss, grad = mse_loss_and_grad(pb, flat, x, t, n_global=n_global)
    net = tr.build_network(list(pb.layers), pb.activation, torch.float64, pb.net_kind)
    tr.set_flat(net, flat)
    X = torch.as_tensor(x)
    out = net(X)
    if pb.envelope == go.ENV_SIN:
        out = out * torch.sin(math.pi * X[:, :1] / pb.env_L)
    tl = ((out - torch.as_tensor(t)) ** 2).sum() / ((n_global or N) * pb.n_out)
    tl.backward()
    tl = float(tl.detach())
    assert abs(loss - tl) <= 1e-10 * tl
    assert H.rel_err(grad, tr.get_flat_grad(net)) <= 1e-10


def test_shards_add_up():
    """two shards with n_global = N: losses and gradients add up to the one-set reference"""
    s = MC.setup("2d_64x4", 333)
    a = mse_loss_and_grad(s["pb"], s["flat"], s["x"][:17], s["target"][:17], n_global=333)
    b = mse_loss_and_grad(s["pb"], s["flat"], s["x"][17:], s["target"][17:], n_global=333)
    assert abs(a[0] + b[0] - s["loss"]) <= 1e-13 * s["loss"]
    assert H.rel_err(a[1] + b[1], s["grad"]) <= 1e-13


@pytest.mark.parametrize("name,N", sorted({(n, N) for n, N, _ in MC.CELLS}), ids=lambda v: str(v))
def test_float32_reference_reaches_the_per_block_bound(name, N):
    s = MC.setup(name, N)
    worst = max(s["f32_blocks"], key=s["f32_blocks"].get)
    print(f"[{name} N={N}] float32 reference: loss {s['f32_loss']:.2e} grad {s['f32_whole']:.2e} worst block {worst} {s['f32_blocks'][worst]:.2e}")
    assert np.isfinite(s["grad"]).all() and s["loss"] > 0
    assert s["f32_blocks"][worst] < 1e-5, s["f32_blocks"]
    assert s["f32_whole"] < 1e-5
    # every block carries a share of the gradient: none vanishes against the whole vector's maximum
    gmax = np.abs(s["grad"]).max()
    share = {nm: np.abs(s["grad"][ix]).max() / gmax for nm, ix in s["blocks"]}
    assert min(share.values()) > 1e-3, share
