"""CPU: tests/mixture_ref.py (the fp64 reference the GPU mixture tests are judged against) held to three independent things:
  1. torch autograd in fp64 with mu_a ATTACHED to the graph (quirk Q10 carries over: each mu_a is its component's own Rayleigh quotient,
     d loss / d mu_a = -2 w_pde / N sum r_a u_a = 0) -- loss and mu_a to 1e-12, gradient to 1e-10 of max|g|, the bars of test_oracle_autograd.py;
  2. decoupling: g12 = 0, n_a = 1 is two scalar problems of oracle.full_loss_and_grad on the networks with the last layer cut to row a;
  3. the inputs of the GPU cases: with the cross term of the seeds deleted the gradient is off by at least 1e-2 of max|g|.
And the sharded two-phase form equals the single call on cuts (1, 17, N - 18)."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import gpe_oracle as go
from oracle import torch_ref as tr
from tests import mixture_cases as mc
from tests import mixture_ref as mr

# name: (layers, N, activation, weighted)
AUTOGRAD = {
    "1d_tanh": ([1, 16, 16, 2], 40, 0, False),
    "1d_shifted_weighted": ([1, 12, 12, 12, 2], 33, 1, True),
    "2d_tanh_weighted": ([2, 16, 16, 16, 2], 45, 0, True),
    "2d_shifted": ([2, 12, 12, 2], 37, 1, False),
    "3d_tanh": ([3, 12, 12, 2], 30, 0, False),
    "3d_shifted_weighted": ([3, 10, 10, 10, 2], 25, 1, True),
}


def _inputs(layers, N, weighted, seed=0):
    rng = np.random.default_rng(seed)
    d = layers[0]
    x = np.linspace(-3, 3, N).reshape(-1, 1) if d == 1 else rng.uniform(-2.5, 2.5, (N, d))
    flat = rng.normal(0, 1, go.param_count(layers)) * 0.4
    x_bc = rng.uniform(-2.5, 2.5, (5, d))
    tgt = rng.normal(0, 0.1, (5, 2))
    q = rng.uniform(0.2, 2.0, N) if weighted else None
    return x, flat, x_bc, tgt, q


def _autograd(mp, flat, x, x_bc, tgt, q):
    """loss, (mu_1, mu_2), gradient by torch: the network is nn.Sequential, derivatives are autograd.grad twice per coordinate, mu_a stay
    in the graph"""
    pb = mp.pb
    net = tr.build_network(list(pb.layers), pb.activation, torch.float64)
    tr.set_flat(net, flat)
    X = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    N, d = x.shape
    qt = torch.ones(N, dtype=torch.float64) if q is None else torch.tensor(q, dtype=torch.float64)
    W = qt.sum()
    out = pb.perturb_scale * net(X)
    V = torch.tensor(go.potential(pb, x), dtype=torch.float64)
    g = [[mp.g[0], mp.g[2]], [mp.g[2], mp.g[1]]]
    u = [out[:, 0], out[:, 1]]
    loss = 0.0
    mus = []
    for a in range(2):
        g1 = torch.autograd.grad(u[a].sum(), X, create_graph=True)[0]
        lap = 0.0
        for k in range(d):
            lap = lap + torch.autograd.grad(g1[:, k].sum(), X, create_graph=True)[0][:, k]
        Hu = -pb.kinetic_coeff * lap + V * u[a] + (g[a][0] * u[0] ** 2 + g[a][1] * u[1] ** 2) * u[a]
        mu = (qt * u[a] * Hu).sum() / (qt * u[a] ** 2).sum()
        r = Hu - mu * u[a]
        I = pb.dx * (qt * u[a] ** 2).sum()
        loss = loss + pb.w_pde * (qt * r * r).sum() / W + pb.w_norm * (I - mp.n[a]) ** 2
        mus.append(float(mu.detach()))
    eb = pb.bc_nn_scale * net(torch.tensor(x_bc, dtype=torch.float64)) - torch.tensor(tgt, dtype=torch.float64)
    loss = loss + pb.w_bc * (eb * eb).mean()
    loss.backward()
    return float(loss.detach()), mus, tr.get_flat_grad(net)


@pytest.mark.parametrize("name", sorted(AUTOGRAD))
def test_reference_matches_autograd_with_mu_attached(name):
    layers, N, act, weighted = AUTOGRAD[name]
    x, flat, x_bc, tgt, q = _inputs(layers, N, weighted)
    mp = mc.problem(layers, N, act, dx=0.05)
    sc, grad, _ = mr.loss_and_grad(mp, flat, x, x_bc, tgt, q=q)
    tl, tmu, tgrad = _autograd(mp, flat, x, x_bc, tgt, q)
    assert abs(tl - sc["loss"]) <= 1e-12 * abs(sc["loss"])
    assert abs(tmu[0] - sc["mu1"]) <= 1e-12 * abs(sc["mu1"]) and abs(tmu[1] - sc["mu2"]) <= 1e-12 * abs(sc["mu2"])
    assert np.abs(tgrad - grad).max() <= 1e-10 * np.abs(grad).max()
    # (the inputs exercise what they claim to: both norm terms and the boundary term are alive, the components differ)
    assert sc["bc"] > 0 and sc["norm"] > 0 and sc["mu1"] != sc["mu2"]


def _row_net(flat, layers, a):
    """the network with the last layer cut to output row a: (flat, layers) of the scalar problem"""
    params = go.unflatten(np.asarray(flat, np.float64), layers)
    W, b = params[-1]
    cut = params[:-1] + [(W[a:a + 1], b[a:a + 1])]
    return go.flatten(cut), list(layers[:-1]) + [1]


@pytest.mark.parametrize("layers,N,act", [([1, 16, 16, 2], 40, 1), ([2, 12, 12, 12, 2], 37, 0), ([3, 10, 10, 2], 25, 0)])
def test_decoupled_mixture_is_two_scalar_problems(layers, N, act):
    """g12 = 0, n_a = 1, w_bc = 0 (the boundary mean's cnt carries the factor n_out): loss = loss_1 + loss_2; the gradient of the hidden
    layers adds, the output rows are each component's own."""
    x, flat, _, _, _ = _inputs(layers, N, False, seed=1)
    g = (1.5, 0.7, 0.0)
    mp = mc.problem(layers, N, act, g=g, norms=(1.0, 1.0), dx=0.05, w_bc=0.0)
    sc, grad, f = mr.loss_and_grad(mp, flat, x)
    blocks = go.unflatten(np.arange(go.param_count(layers)), layers)
    want = np.zeros_like(grad)
    loss = 0.0
    for a in range(2):
        fa, la = _row_net(flat, layers, a)
        pba = dataclasses.replace(mp.pb, layers=la, gamma=g[a])
        sa, ga, ra = go.full_loss_and_grad(pba, fa, x)
        loss += sa["loss"]
        assert abs(sa["mu"] - sc[f"mu{a + 1}"]) <= 1e-12 * abs(sa["mu"])
        np.testing.assert_allclose(f["psi"][:, a], ra["psi"][:, 0], rtol=0, atol=1e-13)
        ia = go.unflatten(np.arange(go.param_count(la)), la)
        for j in range(len(blocks) - 1):                       # hidden layers: the two scalar gradients add
            for full, part in zip(blocks[j], ia[j]):
                want[full.ravel()] += ga[part.ravel()]
        want[blocks[-1][0][a]] = ga[ia[-1][0][0]]                # output layer: row a of the weights, entry a of the bias
        want[blocks[-1][1][a]] = ga[ia[-1][1][0]]
    assert abs(loss - sc["loss"]) <= 1e-12 * abs(sc["loss"])
    assert np.abs(want - grad).max() <= 1e-12 * np.abs(grad).max()


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_gpu_inputs_are_sensitive_to_the_cross_term(name):
    """A condition on the inputs, not a measurement: the GPU cases hold the gradient to 5e-5, so a kernel without the cross term must be
    off by far more than that on them."""
    mp, x, flat, x_bc, tgt, _ = mc.case(name)
    args = (mp, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64), tgt.astype(np.float64))
    good = mr.loss_and_grad(*args)[1]
    bad = mr.loss_and_grad(*args, drop_cross=True)[1]
    assert np.abs(bad - good).max() >= 1e-2 * np.abs(good).max()


@pytest.mark.parametrize("layers,N,weighted", [([2, 16, 16, 2], 60, False), ([1, 12, 12, 2], 45, True), ([3, 10, 10, 2], 40, True)])
def test_sharded_equals_the_single_call(layers, N, weighted):
    x, flat, x_bc, tgt, q = _inputs(layers, N, weighted, seed=2)
    mp = mc.problem(layers, N, 0, dx=0.05)
    sc, grad, _ = mr.loss_and_grad(mp, flat, x, x_bc, tgt, q=q)
    sc2, grad2 = mr.sharded_loss_and_grad(mp, flat, x, (1, 17, N - 18), x_bc, tgt, q=q)
    for k in ("loss", "pde", "bc", "norm", "mu1", "mu2", "integral1", "integral2"):
        assert abs(sc[k] - sc2[k]) <= 1e-12 * max(1.0, abs(sc[k])), k
    assert np.abs(grad - grad2).max() <= 1e-12 * np.abs(grad).max()
