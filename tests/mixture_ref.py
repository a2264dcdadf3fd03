"""fp64 reference of the two-component mixture step (include/gpe_hip.h: gpe_config.mixture).  The network and its reverse pass are the
oracle's (mlp_forward / mlp_backward); head, seeds and loss are written out here:

  H_a u_a = -c lap u_a + V u_a + (g_a1 u_1^2 + g_a2 u_2^2) u_a,   mu_a = sum q u_a H_a u_a / sum q u_a^2,   I_a = dx sum q u_a^2
  loss = w_pde sum q (r_1^2 + r_2^2) / W + w_norm sum_a (I_a - n_a)^2 + w_bc mean(e_bc^2),   r_a = H_a u_a - mu_a u_a

with mu_a held constant in the reverse pass (its branch vanishes: tests/test_mixture_reference_cpu.py holds the gradient to torch
autograd with mu_a attached to the graph).  q: optional per-point quadrature weights, W = sum q over all ranks (without weights q = 1,
W = N).  Two-phase form for data-parallel shards: local_sums() per shard, added by the caller, then loss_and_grad(totals=...)."""
import dataclasses

import numpy as np

from oracle import gpe_oracle as go

SUM_KEYS = ("num1", "den1", "num2", "den2")


@dataclasses.dataclass
class MixProblem:
    pb: go.Problem                     # network, potential, kinetic_coeff, perturb_scale, bc_nn_scale, dx, n_global, the loss weights
    g: tuple                           # (g11, g22, g12)
    n: tuple = (1.0, 1.0)              # target norms (n_1, n_2)


def _head(mp, params, x):
    pb = mp.pb
    d = x.shape[1]
    out, cache = go.mlp_forward(params, x, pb.activation)
    U = pb.perturb_scale * out                                   # [C, N, 2]
    u = U[0]
    lap = U[1 + d:1 + 2 * d].sum(axis=0)
    V = go.potential(pb, x)
    g11, g22, g12 = (float(v) for v in mp.g)
    s1, s2 = u[:, 0] ** 2, u[:, 1] ** 2
    Hu = -pb.kinetic_coeff * lap + V[:, None] * u
    Hu[:, 0] += (g11 * s1 + g12 * s2) * u[:, 0]
    Hu[:, 1] += (g12 * s1 + g22 * s2) * u[:, 1]
    return u, Hu, V, cache


def _sums(u, Hu, q):
    return dict(num1=float((q * u[:, 0] * Hu[:, 0]).sum()), den1=float((q * u[:, 0] ** 2).sum()),
                num2=float((q * u[:, 1] * Hu[:, 1]).sum()), den2=float((q * u[:, 1] ** 2).sum()))


def local_sums(mp, flat, x, q=None):
    """phase 1 on a shard: the four Rayleigh sums of its points"""
    x = np.asarray(x, np.float64)
    q = np.ones(x.shape[0]) if q is None else np.asarray(q, np.float64).ravel()
    params = go.unflatten(np.asarray(flat, np.float64), mp.pb.layers)
    u, Hu, _, _ = _head(mp, params, x)
    return _sums(u, Hu, q)


def loss_and_grad(mp, flat, x, x_bc=None, bc_target=None, q=None, W=None, totals=None, drop_cross=False, world=1):
    """-> (scalars, gradient, fields).  totals: the four sums over ALL shards (None: this batch's own); W: N of the means (None:
    pb.n_global, else sum q / the row count); the boundary term is replicated over `world` shards, so a shard adds 1/world of its
    gradient.  scalars: loss, pde, bc, norm, mu1, mu2, integral1, integral2, sum_r2 (this shard's) and the four sums (the totals used).
    drop_cross: leave the cross term rb_b 2 g_12 u_a u_b out of the seeds (a deliberately WRONG gradient, for the sensitivity test)."""
    pb = mp.pb
    x = np.asarray(x, np.float64)
    N, d = x.shape
    q = np.ones(N) if q is None else np.asarray(q, np.float64).ravel()
    if W is None:
        W = float(pb.n_global) if pb.n_global > 0 else float(q.sum())
    flat = np.asarray(flat, np.float64)
    params = go.unflatten(flat, pb.layers)
    u, Hu, V, cache = _head(mp, params, x)
    tot = _sums(u, Hu, q) if totals is None else totals
    mu = np.array([tot["num1"] / tot["den1"], tot["num2"] / tot["den2"]])
    I = np.array([tot["den1"], tot["den2"]]) * pb.dx
    nt = np.array([float(v) for v in mp.n])
    r = Hu - mu[None, :] * u
    sr2 = float((q[:, None] * r * r).sum())
    g11, g22, g12 = (float(v) for v in mp.g)
    rb = (2.0 * pb.w_pde / W) * r
    s1, s2 = u[:, 0] ** 2, u[:, 1] ** 2
    cross = 0.0 if drop_cross else 2.0 * g12 * u[:, 0] * u[:, 1]
    ub = np.empty_like(u)
    ub[:, 0] = rb[:, 0] * (V + 3 * g11 * s1 + g12 * s2 - mu[0]) + rb[:, 1] * cross
    ub[:, 1] = rb[:, 1] * (V + 3 * g22 * s2 + g12 * s1 - mu[1]) + rb[:, 0] * cross
    ub += 4.0 * pb.w_norm * (I - nt)[None, :] * pb.dx * u
    Ub = np.zeros((1 + 2 * d, N, 2))
    Ub[0] = ub
    for k in range(d):
        Ub[1 + d + k] = -pb.kinetic_coeff * rb
    grad = go.mlp_backward(params, cache, pb.perturb_scale * q[None, :, None] * Ub)
    L_bc = 0.0
    if x_bc is not None and pb.w_bc != 0.0:
        ob, cb = go.mlp_forward(params, np.asarray(x_bc, np.float64), pb.activation, value_only=True)
        eb = pb.bc_nn_scale * ob[0]
        if bc_target is not None:
            eb = eb - np.asarray(bc_target, np.float64).reshape(eb.shape)
        L_bc = float((eb * eb).mean())                            # cnt = n_bc * n_out
        ebar = (pb.w_bc * 2.0 / eb.size) * eb * pb.bc_nn_scale / world
        grad = grad + go.mlp_backward(params, cb, ebar[None], value_only=True)
    norm = float(((I - nt) ** 2).sum())
    sc = dict(pde=sr2 / W, bc=L_bc, norm=norm, mu1=float(mu[0]), mu2=float(mu[1]), integral1=float(I[0]), integral2=float(I[1]),
              sum_r2=sr2, **{k: float(tot[k]) for k in SUM_KEYS})
    sc["loss"] = pb.w_pde * sc["pde"] + pb.w_bc * L_bc + pb.w_norm * norm
    return sc, grad, dict(psi=u, Hu=Hu, residual=r)


def sharded_loss_and_grad(mp, flat, x, cuts, x_bc=None, bc_target=None, q=None):
    """The data-parallel protocol on contiguous shards with the given row counts: phase 1 per shard, totals, phase 2 per shard with the
    totals; every shard carries the replicated boundary batch at 1 / world.  -> (scalars, gradient) of the whole batch."""
    x = np.asarray(x, np.float64)
    q = np.ones(x.shape[0]) if q is None else np.asarray(q, np.float64).ravel()
    assert sum(cuts) == x.shape[0]
    W = float(mp.pb.n_global) if mp.pb.n_global > 0 else float(q.sum())
    edges = np.concatenate([[0], np.cumsum(cuts)])
    sl = [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
    parts = [local_sums(mp, flat, x[s], q[s]) for s in sl]
    tot = {k: float(sum(p[k] for p in parts)) for k in SUM_KEYS}
    res = [loss_and_grad(mp, flat, x[s], x_bc, bc_target, q=q[s], W=W, totals=tot, world=len(sl)) for s in sl]
    sc = dict(res[0][0])
    sc["sum_r2"] = float(sum(r[0]["sum_r2"] for r in res))
    sc["pde"] = sc["sum_r2"] / W
    sc["loss"] = mp.pb.w_pde * sc["pde"] + mp.pb.w_bc * sc["bc"] + mp.pb.w_norm * sc["norm"]
    return sc, sum(r[1] for r in res)
