"""Tables of analytic potential terms and fixed-seed points shared by tests/test_potential_terms_cpu.py (the host instance of the
evaluator, under the sanitizers) and tests/test_gpu_potential_terms.py (the device instance and the engine around it).  numpy only."""
import numpy as np

from gpe_pinn import potential as pot


def single(kind, dim):
    """one term of `kind` with an off-centre, anisotropic (w, c) on `dim` axes"""
    w = (0.9, 1.3, 0.6)[:dim]
    c = (0.4, -0.7, 0.25)[:dim]
    return {"quadratic": [pot.quadratic(0.5, w, c)],
            "quartic": [pot.quartic(0.02, w, c)],
            "gaussian": [pot.gaussian(-3.0, w, c)],
            "lattice": [pot.lattice(2.5, (2.2, 0.0, 1.7)[:dim], c)],
            "linear": [pot.linear(0.3, w, c)]}[kind]


# U of potential.error_bound on the device: the error of expf / cosf THEMSELVES in ulp.  The HIP math documentation is not part of the ROCm
# install, so it is measured: tools/potential_ulp.py, over the fixed inputs of tests/test_gpu_potential_terms.py, single-term GAUSS and LATTICE
# tables, with the argument taken as the device forms it (t_k and s are correctly rounded fp32 operations, restated bit for bit) -- 0.35 ulp
# at most (profiles/potential/values_ulp.txt), doubled for another compiler's contraction choices, rounded up.  The error of the whole TERM
# against the fp64 reference, in ulp of V, is a different and far larger figure (up to 2374 ulp in that file): it is mostly the rounding of
# the argument (s ~ 30 multiplies it by 30; cos^2 near a zero has a tiny ulp), which error_bound counts in its own (dim + 3) s and 6 |t_k|
# parts; taken for U it would make the bound vacuous.
U_DEVICE = 1.0

SAMPLER_SEED = 11
KINDS = ("quadratic", "quartic", "gaussian", "lattice", "linear")


def mix16(dim):
    """sixteen terms, every kind more than once, amplitudes of both signs"""
    rng = np.random.default_rng(1600 + dim)
    make = (pot.quadratic, pot.quartic, pot.gaussian, pot.lattice, pot.linear)
    scale = (0.5, 0.01, 2.0, 1.5, 0.2)
    out = []
    for j in range(16):
        k = j % 5
        w = rng.uniform(0.4, 1.6, dim)
        c = rng.uniform(-1.0, 1.0, dim)
        a = scale[k] * rng.uniform(0.5, 1.5) * (-1.0 if j % 3 == 2 else 1.0)
        out.append(make[k](a, w, c))
    return out


def trap4(dim):
    """the four-term trap of the sampler tests: a tilted anisotropic trap, a Gaussian dimple, a weak quartic wall, an optical lattice"""
    w = (1.0, 1.4, 0.8)[:dim]
    return [pot.quadratic(0.5, w, (0.3, -0.2, 0.1)[:dim]), pot.gaussian(-2.0, (1.2,) * dim, (-0.5, 0.4, 0.0)[:dim]),
            pot.quartic(0.01, (1.0,) * dim), pot.lattice(1.5, (2.0,) + (0.0,) * (dim - 1))]


def redraw_table(dim=2):
    """the table of the redraw tests: a trap, a dimple, a quartic wall and a deep lattice on every axis whose period is a few cells of the
    sampler grids (deeper in 1D, where the class's state is mostly its analytic base and a shallow lattice moves the loss little), so that V of
    one draw is far from V of the next (tests/test_potential_terms_cpu.py holds that to the oracle)"""
    return [pot.quadratic(0.5, (1.0, 1.4, 0.8)[:dim], (0.3, -0.2, 0.1)[:dim]), pot.gaussian(-2.0, (1.2,) * dim, (-0.5, 0.4, 0.0)[:dim]),
            pot.quartic(0.01, (1.0,) * dim), pot.lattice({1: 40.0, 2: 8.0, 3: 8.0}[dim], (3.0, 2.5, 2.0)[:dim], (0.1, -0.2, 0.3)[:dim])]


def weighted_loss_and_grad(pb, flat, x, q, V, W=None, orth=None):
    """tests/weighted_ref.py's reference -- the oracle's two-phase protocol with ONE point per shard, sums and gradient weighted by q_i, N of
    the means W -- with a precomputed potential: point i is handed V_pre = V[i:i+1].  No boundary rows.  -> (scalars, gradient)"""
    import dataclasses
    from oracle import gpe_oracle as go
    x, q, V, flat = (np.asarray(a, np.float64) for a in (x, np.ravel(q), np.ravel(V), flat))
    N = x.shape[0]
    assert q.shape == V.shape == (N,) and np.all(q >= 0)
    W = float(q.sum()) if W is None else float(W)
    pbw = dataclasses.replace(pb, n_global=W)
    sl = (lambda i: None) if orth is None else (lambda i: np.asarray(orth, np.float64)[:, i:i + 1])
    parts = [go.loss_and_grad(pbw, flat, x[i:i + 1], V_pre=V[i:i + 1], orth=sl(i), phase=1) for i in range(N)]
    tot = {k: float(sum(q[i] * parts[i][k] for i in range(N))) for k in parts[0]}
    grad, sr2, res0 = None, 0.0, None
    for i in range(N):
        r = go.loss_and_grad(pbw, flat, x[i:i + 1], V_pre=V[i:i + 1], orth=sl(i), shard_sums=tot)
        if i == 0:
            res0, grad = r, r["grad_bc"].copy()
        grad += q[i] * r["grad_local"]
        sr2 += q[i] * r["sum_r2"]
    sc = go.assemble(pbw, res0, sum_r2_total=sr2, n_global=W)
    return sc, grad


def live_tables(dim):
    """(before, after) of the live change: a trap with an optical lattice whose depth is tripled"""
    w = (1.0, 1.4, 0.8)[:dim]
    base = [pot.quadratic(0.5, w, (0.3, -0.2, 0.1)[:dim]), pot.gaussian(-2.0, (1.2,) * dim, (-0.5, 0.4, 0.0)[:dim])]
    lat = pot.lattice(4.0, (2.0,) + (0.0,) * (dim - 1))
    return base + [lat], base + [lat._replace(a=3.0 * lat.a)]


def points(dim, n, seed=0, half=4.0):
    return np.random.default_rng(9000 + 10 * dim + seed).uniform(-half, half, (n, dim)).astype(np.float32)


def ulp_error(got32, ref64):
    """|got - ref| in units of the float32 ulp of ref"""
    ref64 = np.asarray(ref64, np.float64)
    ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got32, np.float64) - ref64) / ulp
