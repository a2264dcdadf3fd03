"""Reference of the pre-training (MSE) step's loss and gradient, built only from oracle.gpe_oracle: what gpe_mse_begin computes with
k_seed_mse (csrc/gpe_head.h) behind the value-only forward pass and in front of the value-only reverse pass.

    o     = NN(x)                                   value-only forward, [N, n_out]
    f     = sin(pi x_0 / env_L) for ENV_SIN, else 1 (model.forward includes the boundary factor)
    e     = f o - t                                 t [N, n_out]
    loss  = sum(e^2) / (n_global n_out)             n_global = N unless the points are one shard of a larger set
    o_bar = 2 / (n_global n_out) e f                seeds of the reverse pass

The loss is unweighted whatever quadrature weights are bound.  No torch, no HIP: a checker in the dtype asked for (float64 by default;
float32 shows what fp32 arithmetic can reach on the same inputs, tests/test_mse_reference_cpu.py)."""
import math

import numpy as np

from oracle import gpe_oracle as go


def mse_loss_and_grad(pb, flat, x, target, n_global=None, dtype=np.float64):
    """-> (loss, flat gradient in the layout of go.unflatten) of mean((f NN(x) - target)^2) over n_global * n_out values"""
    dt = np.dtype(dtype)
    x = np.asarray(x, dt).reshape(-1, pb.dim)
    N, n_out = x.shape[0], pb.n_out
    t = np.asarray(target, dt).reshape(N, n_out)
    n_global = N if n_global is None else int(n_global)
    params = go.unflatten(np.asarray(flat, dt), pb.layers, pb.net_kind)
    _, skip, plain = go.expand_layers(pb.layers, pb.net_kind)
    out, cache = go.mlp_forward(params, x, pb.activation, value_only=True, skip=skip, plain_tanh=plain)
    f = np.sin(dt.type(math.pi / pb.env_L) * x[:, :1]) if pb.envelope == go.ENV_SIN else np.ones((N, 1), dt)
    e = f * out[0] - t
    loss = float(np.sum(e * e, dtype=np.float64)) / (n_global * n_out)
    seed = (dt.type(2.0 / (n_global * n_out)) * e * f)[None]
    grad = go.mlp_backward(params, cache, seed, value_only=True, skip=skip)
    return loss, grad
