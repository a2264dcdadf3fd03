"""The oracle on a seam cell (tests/seam_table.py), in float64 (the reference of tests/test_gpu_seams.py) or in float32 (its own
rounding, tests/test_seam_table_cpu.py): one call on the whole batch up to 65 536 points, go.sharded_loss_and_grad beyond."""
import numpy as np

from oracle import gpe_oracle as go
from tests import seam_table as S

SHARD_FROM = 65536


def problem(cls):
    return go.Problem(**S.CLASSES[cls][0])


def step(cls, n, dtype=np.float64):
    """(scalars, gradient) of the class's step on n bound points"""
    pb = problem(cls)
    x, flat, x_bc = S.inputs(cls, n)
    a = (flat.astype(dtype), x.astype(dtype), x_bc.astype(dtype))
    if n > SHARD_FROM:
        return go.sharded_loss_and_grad(pb, *a, chunk=65536, threads=8)
    sc, grad, _ = go.full_loss_and_grad(pb, *a)
    return sc, grad


def fields(cls, n, mu):
    """(output jets [C, n, n_out], psi, residual field) in float64, chunked; the residual with the step's eigenvalue mu"""
    pb = problem(cls)
    x, flat, _ = S.inputs(cls, n)
    params = go.unflatten(flat.astype(np.float64), pb.layers, pb.net_kind)
    _, skip, plain = go.expand_layers(pb.layers, pb.net_kind)
    jets, psi, res = [], [], []
    for a in range(0, n, SHARD_FROM):
        xc = x[a:a + SHARD_FROM].astype(np.float64)
        out, _ = go.mlp_forward(params, xc, pb.activation, skip=skip, plain_tanh=plain)
        h = go.head_pde(pb, xc, out)
        jets.append(out); psi.append(h["u"]); res.append(h["Hu"] - mu * h["u"])
    return np.concatenate(jets, axis=1), np.concatenate(psi), np.concatenate(res)
