"""fp64 reference of the mixture step with its energy term (include/gpe_hip.h: gpe_mixture_energy_weight).  tests/mixture_ref.py, imported
unchanged, gives head, residual seeds and the plain loss; this module adds

  T_a = sum q (c |grad u_a|^2 + V u_a^2),   Q_ab = sum q u_a^2 u_b^2,   den_a = sum q u_a^2
  E = sum_a n_a T_a / den_a + 1/2 sum_ab g_ab n_a n_b Q_ab / (den_a den_b dx),        loss += w_E E

the energy of the state normalised to the target norms, v_a = u_a sqrt(n_a / I_a), and its seeds at the output jets

  d/du_a = 2 alpha_a V u_a + 4 beta_aa u_a^3 + 2 beta_12 u_a u_b^2 + 2 delta_a u_a ,   d/d(d_k u_a) = 2 c alpha_a d_k u_a

(alpha_a = n_a / den_a, beta_aa = 1/2 g_aa n_a^2 / (den_a^2 dx), beta_12 = g_12 n_1 n_2 / (den_1 den_2 dx), delta_a = dE / d den_a).
tests/test_mixture_energy_reference_cpu.py holds the gradient to torch autograd of E written directly on v_a.  The two-phase sharded form
carries nine sums: the four Rayleigh sums of mixture_ref and T_1, T_2, Q_11, Q_22, Q_12."""
import numpy as np

from oracle import gpe_oracle as go
from tests import mixture_ref as mr

ENERGY_KEYS = ("T1", "T2", "Q11", "Q22", "Q12")
SUM_KEYS = mr.SUM_KEYS + ENERGY_KEYS
ENERGY_FIELDS = ("E", "T1", "T2", "Q11", "Q22", "Q12", "den1", "den2")        # Engine.mixture_energy()

# w_E of the GPU tests per case of tests/mixture_cases.py.  The residual gradient of these random networks spans 28 .. 81 000 between the
# cases and the gradient of E 0.16 .. 14, so one weight cannot serve them all: each is the power of two next to 2 max|g_plain| / max|g_E|,
# at which the energy term carries about half of max|g| and the plain terms the rest -- a wrong energy seed AND a wrong residual seed of
# the energy instances both miss the 5e-5 bound.  tests/test_mixture_energy_reference_cpu.py asserts on these inputs and weights that the
# gradient moves by at least 1 % of max|g| without the delta_a term and without the first-derivative seeds (measured: >= 1.7 and >= 0.026).
W_E = {
    "fused_2d_64x3_N37": 32768.0,
    "fused_2d_64x3_N49": 1024.0,
    "fused_2d_64x3_N1025": 512.0,
    "fused_2d_32x3_N37": 131072.0,
    "fused_2d_128x2_N1025": 16.0,
    "padded_2d_72x3_N37": 128.0,
    "wide_3d_256x2_N300": 16.0,
    "generic_1d_48x2_N37": 16384.0,
    "generic_2d_64x2_N1025": 1024.0,
    "generic_3d_40_N37": 8192.0,
}


def _jets(mp, flat, x):
    """u [N, 2], grad u [d, N, 2], V [N], and what mlp_backward needs"""
    pb = mp.pb
    params = go.unflatten(np.asarray(flat, np.float64), pb.layers)
    out, cache = go.mlp_forward(params, x, pb.activation)
    U = pb.perturb_scale * out
    d = x.shape[1]
    return U[0], U[1:1 + d], go.potential(pb, x), params, cache


def _energy_sums(mp, u, du, V, q):
    c = mp.pb.kinetic_coeff
    s = u * u
    T = (q[:, None] * (c * (du * du).sum(axis=0) + V[:, None] * s)).sum(axis=0)
    return dict(T1=float(T[0]), T2=float(T[1]), Q11=float((q * s[:, 0] ** 2).sum()), Q22=float((q * s[:, 1] ** 2).sum()),
                Q12=float((q * s[:, 0] * s[:, 1]).sum()))


def local_sums(mp, flat, x, q=None):
    """phase 1 on a shard: the nine sums of its points"""
    x = np.asarray(x, np.float64)
    q = np.ones(x.shape[0]) if q is None else np.asarray(q, np.float64).ravel()
    u, du, V, _, _ = _jets(mp, flat, x)
    return dict(mr.local_sums(mp, flat, x, q), **_energy_sums(mp, u, du, V, q))


def energy_of(mp, tot):
    """-> (E, alpha [2], beta (11, 22, 12), delta [2]) from the nine sums over all shards"""
    g11, g22, g12 = (float(v) for v in mp.g)
    n1, n2 = (float(v) for v in mp.n)
    d1, d2, dx = tot["den1"], tot["den2"], mp.pb.dx
    alpha = (n1 / d1, n2 / d2)
    beta = (0.5 * g11 * n1 * n1 / (d1 * d1 * dx), 0.5 * g22 * n2 * n2 / (d2 * d2 * dx), g12 * n1 * n2 / (d1 * d2 * dx))
    E = alpha[0] * tot["T1"] + alpha[1] * tot["T2"] + beta[0] * tot["Q11"] + beta[1] * tot["Q22"] + beta[2] * tot["Q12"]
    delta = (-(alpha[0] * tot["T1"] + 2.0 * beta[0] * tot["Q11"] + beta[2] * tot["Q12"]) / d1,
             -(alpha[1] * tot["T2"] + 2.0 * beta[1] * tot["Q22"] + beta[2] * tot["Q12"]) / d2)
    return E, alpha, beta, delta


def loss_and_grad(mp, w_E, flat, x, x_bc=None, bc_target=None, q=None, W=None, totals=None, world=1, drop_delta=False, drop_first=False):
    """mixture_ref.loss_and_grad plus w_E E -> (scalars, gradient, fields).  scalars gain E (also under 'riesz', where the engine's record
    reports it) and the five energy sums; loss includes w_E E.  totals: the nine sums over ALL shards.  drop_delta / drop_first: leave the
    2 delta_a u_a term / the first-derivative seeds out (deliberately WRONG gradients, for the sensitivity test)."""
    pb = mp.pb
    x = np.asarray(x, np.float64)
    N, d = x.shape
    q = np.ones(N) if q is None else np.asarray(q, np.float64).ravel()
    flat = np.asarray(flat, np.float64)
    sc, grad, fields = mr.loss_and_grad(mp, flat, x, x_bc, bc_target, q=q, W=W, totals=totals, world=world)
    u, du, V, params, cache = _jets(mp, flat, x)
    tot = dict({k: sc[k] for k in mr.SUM_KEYS}, **(_energy_sums(mp, u, du, V, q) if totals is None else {k: totals[k] for k in ENERGY_KEYS}))
    E, alpha, beta, delta = energy_of(mp, tot)
    s = u * u
    Ub = np.zeros((1 + 2 * d, N, 2))
    for a in range(2):
        b = 1 - a
        Ub[0, :, a] = 2.0 * alpha[a] * V * u[:, a] + 4.0 * beta[a] * s[:, a] * u[:, a] + 2.0 * beta[2] * u[:, a] * s[:, b]
        if not drop_delta:
            Ub[0, :, a] += 2.0 * delta[a] * u[:, a]
        if not drop_first:
            Ub[1:1 + d, :, a] = 2.0 * pb.kinetic_coeff * alpha[a] * du[:, :, a]
    grad = grad + go.mlp_backward(params, cache, float(w_E) * pb.perturb_scale * q[None, :, None] * Ub)
    sc = dict(sc, E=E, riesz=E, **{k: float(tot[k]) for k in ENERGY_KEYS})
    sc["loss"] = sc["loss"] + float(w_E) * E
    return sc, grad, fields


def energy_fields(sc):
    """the eight numbers Engine.mixture_energy() returns, from the reference's scalars"""
    return {k: sc[k] for k in ENERGY_FIELDS}


def sharded_loss_and_grad(mp, w_E, flat, x, cuts, x_bc=None, bc_target=None, q=None):
    """mixture_ref.sharded_loss_and_grad with the nine sums in the first exchange -> (scalars, gradient) of the whole batch"""
    x = np.asarray(x, np.float64)
    q = np.ones(x.shape[0]) if q is None else np.asarray(q, np.float64).ravel()
    assert sum(cuts) == x.shape[0]
    W = float(mp.pb.n_global) if mp.pb.n_global > 0 else float(q.sum())
    edges = np.concatenate([[0], np.cumsum(cuts)])
    sl = [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
    parts = [local_sums(mp, flat, x[s], q[s]) for s in sl]
    tot = {k: float(sum(p[k] for p in parts)) for k in SUM_KEYS}
    res = [loss_and_grad(mp, w_E, flat, x[s], x_bc, bc_target, q=q[s], W=W, totals=tot, world=len(sl)) for s in sl]
    sc = dict(res[0][0])
    sc["sum_r2"] = float(sum(r[0]["sum_r2"] for r in res))
    sc["pde"] = sc["sum_r2"] / W
    sc["loss"] = mp.pb.w_pde * sc["pde"] + mp.pb.w_bc * sc["bc"] + mp.pb.w_norm * sc["norm"] + float(w_E) * sc["E"]
    return sc, sum(r[1] for r in res)
