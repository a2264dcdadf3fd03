"""CPU: tests/mixture_energy_ref.py (the fp64 reference the GPU tests of the mixture energy term are judged against) and
tests/mixture_flow_1d.py (the yardstick of the demixing test), each held to something independent of it:
  1. torch autograd in fp64 of w_pde pde + w_norm norm + w_bc bc + w_E E[v], E written directly on the normalised v_a = u_a sqrt(n_a / I_a)
     and mu_a attached to the graph: loss and E to 1e-12, gradient to 1e-10 of max|g|;
  2. E does not change with perturb_scale (1 against 0.7) to 1e-12;
  3. g12 = 0, n = (1, 1): E is the sum of two GPE_RIESZ_VARIATIONAL energies of the scalar oracle at p = 3;
  4. the sharded two-phase form equals the single call on cuts (1, 17, N - 18) to 1e-12;
  5. the inputs and weights of the GPU cases: without the delta_a term, and without the first-derivative seeds, the gradient is off by
     at least 1e-2 of max|g|;
  6. the flow: g12 = 0 reproduces oracle/gp_ground_state.py; for g = 10, g12 = 14, n = 1/2 each a symmetric start stays symmetric, a
     separated start ends below it, and both energies are stable under grid doubling to 1e-6."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import gp_ground_state as gs
from oracle import gpe_oracle as go
from oracle import torch_ref as tr
from tests import mixture_cases as mc
from tests import mixture_energy_ref as me
from tests import mixture_flow_1d as mf
from tests.test_mixture_reference_cpu import AUTOGRAD, _inputs, _row_net

W_E_AUTOGRAD = 1024.0          # (the plain gradient of these random networks is 1e2 .. 1e4 times that of E)


def _autograd(mp, w_E, flat, x, x_bc, tgt, q):
    """loss, E, gradient by torch: derivatives are autograd.grad per coordinate, mu_a and the normalisation of v_a stay in the graph"""
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
    v, dv = [], []
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
        s = torch.sqrt(mp.n[a] / I)
        v.append(s * u[a])
        dv.append(s * g1)
    # E[v] = dx sum q (sum_a c |grad v_a|^2 + V v_a^2 + 1/2 sum_ab g_ab v_a^2 v_b^2): the quadrature of the continuum energy
    dens = sum(pb.kinetic_coeff * (dv[a] ** 2).sum(dim=1) + V * v[a] ** 2 for a in range(2))
    dens = dens + 0.5 * sum(g[a][b] * v[a] ** 2 * v[b] ** 2 for a in range(2) for b in range(2))
    E = pb.dx * (qt * dens).sum()
    eb = pb.bc_nn_scale * net(torch.tensor(x_bc, dtype=torch.float64)) - torch.tensor(tgt, dtype=torch.float64)
    loss = loss + pb.w_bc * (eb * eb).mean() + w_E * E
    loss.backward()
    return float(loss.detach()), float(E.detach()), tr.get_flat_grad(net)


@pytest.mark.parametrize("name", sorted(AUTOGRAD))
def test_reference_matches_autograd_of_the_energy_on_the_normalised_state(name):
    layers, N, act, weighted = AUTOGRAD[name]
    x, flat, x_bc, tgt, q = _inputs(layers, N, weighted)
    mp = mc.problem(layers, N, act, dx=0.05)
    sc, grad, _ = me.loss_and_grad(mp, W_E_AUTOGRAD, flat, x, x_bc, tgt, q=q)
    tl, tE, tgrad = _autograd(mp, W_E_AUTOGRAD, flat, x, x_bc, tgt, q)
    assert abs(tE - sc["E"]) <= 1e-12 * abs(sc["E"]) and sc["riesz"] == sc["E"]
    assert abs(tl - sc["loss"]) <= 1e-12 * abs(sc["loss"])
    assert np.abs(tgrad - grad).max() <= 1e-10 * np.abs(grad).max()
    plain = me.loss_and_grad(mp, 0.0, flat, x, x_bc, tgt, q=q)[1]
    assert np.abs(grad - plain).max() > 1e-3 * np.abs(grad).max()         # (the energy term is alive in what was compared)


@pytest.mark.parametrize("name", sorted(AUTOGRAD))
def test_energy_does_not_change_with_the_scale_of_the_state(name):
    layers, N, act, weighted = AUTOGRAD[name]
    x, flat, x_bc, tgt, q = _inputs(layers, N, weighted)
    E = []
    for s in (1.0, 0.7):
        mp = mc.problem(layers, N, act, dx=0.05, perturb_scale=s)
        E.append(me.loss_and_grad(mp, 1.0, flat, x, x_bc, tgt, q=q)[0]["E"])
    assert abs(E[0] - E[1]) <= 1e-12 * abs(E[0])


@pytest.mark.parametrize("layers,N,act", [([1, 16, 16, 2], 40, 1), ([2, 12, 12, 12, 2], 37, 0), ([3, 10, 10, 2], 25, 0)])
def test_decoupled_energy_is_two_scalar_variational_energies(layers, N, act):
    x, flat, _, _, _ = _inputs(layers, N, False, seed=1)
    g = (1.5, 0.7, 0.0)
    mp = mc.problem(layers, N, act, g=g, norms=(1.0, 1.0), dx=0.05, w_bc=0.0)
    sc, _, _ = me.loss_and_grad(mp, 1.0, flat, x)
    E = 0.0
    for a in range(2):
        fa, la = _row_net(flat, layers, a)
        pba = dataclasses.replace(mp.pb, layers=la, gamma=g[a], w_riesz=1.0, riesz_kind=go.RIESZ_VARIATIONAL)
        E += go.full_loss_and_grad(pba, fa, x)[0]["riesz"]
    assert abs(E - sc["E"]) <= 1e-12 * abs(E)


@pytest.mark.parametrize("layers,N,weighted", [([2, 16, 16, 2], 60, False), ([1, 12, 12, 2], 45, True), ([3, 10, 10, 2], 40, True)])
def test_sharded_equals_the_single_call(layers, N, weighted):
    x, flat, x_bc, tgt, q = _inputs(layers, N, weighted, seed=2)
    mp = mc.problem(layers, N, 0, dx=0.05)
    sc, grad, _ = me.loss_and_grad(mp, W_E_AUTOGRAD, flat, x, x_bc, tgt, q=q)
    sc2, grad2 = me.sharded_loss_and_grad(mp, W_E_AUTOGRAD, flat, x, (1, 17, N - 18), x_bc, tgt, q=q)
    for k in ("loss", "pde", "bc", "norm", "mu1", "mu2", "integral1", "integral2", "E") + me.ENERGY_KEYS:
        assert abs(sc[k] - sc2[k]) <= 1e-12 * max(1.0, abs(sc[k])), k
    assert np.abs(grad - grad2).max() <= 1e-12 * np.abs(grad).max()


@pytest.mark.parametrize("name", sorted(me.W_E))
def test_gpu_inputs_are_sensitive_to_both_energy_seeds(name):
    """A condition on the inputs and weights, not a measurement: the GPU cases hold the gradient to 5e-5, so a kernel without the delta_a
    term or without the first-derivative seeds must be off by far more than that on them."""
    mp, x, flat, x_bc, tgt, _ = mc.case(name)
    args = (mp, me.W_E[name], flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64), tgt.astype(np.float64))
    good = me.loss_and_grad(*args)[1]
    for drop in ("drop_delta", "drop_first"):
        bad = me.loss_and_grad(*args, **{drop: True})[1]
        assert np.abs(bad - good).max() >= 1e-2 * np.abs(good).max(), drop
    plain = me.loss_and_grad(args[0], 0.0, *args[2:])[1]                   # ... and the plain terms still carry a fifth of it at least
    assert np.abs(plain).max() >= 0.2 * np.abs(good).max()


# ---- tests/mixture_flow_1d.py ----------------------------------------------------------------------------------------------------------
def test_flow_without_cross_coupling_reproduces_the_scalar_solver():
    """g12 = 0, n = (1, 1): each component is the scalar ground state at its own gamma -- mu_a against the Newton solver on the same grid
    (the same second-order operator: agreement to the solvers' tolerances) and against its Richardson value (to the h^2 term)"""
    g = (10.0, 4.0, 0.0)
    n, half = 1025, 8.0
    x, h = mf.grid(n, half)
    v, E, _ = mf.flow(mf.start(x, (1.0, 1.0), 0.0), x, g, (1.0, 1.0), tol=1e-14)
    mu = mf.chemical_potentials(v, x, g)
    same = gs._solve_on_grid([g[1], g[0]], n, half, 0.5, 0.5, 0)
    lam, _ = gs.ground_state_1d([g[1], g[0]], c=0.5, vscale=0.5, half=half, n=n)
    for a in range(2):
        l, _, u = same[g[a]]
        assert abs(mu[a] - l) <= 1e-6 * l                              # (the flow stops on the energy, which is second order in the state's error)
        assert np.abs(v[:, a] - u).max() <= 1e-6
        assert abs(mu[a] - lam[g[a]]) <= 5e-5 * lam[g[a]]


def test_flow_keeps_the_symmetric_state_and_finds_the_separated_one_below_it():
    g, norms = (10.0, 10.0, 14.0), (0.5, 0.5)
    x, h = mf.grid(1025, 8.0)
    vs, Es, _ = mf.flow(mf.start(x, norms, 0.0), x, g, norms)
    assert np.array_equal(vs[:, 0], vs[:, 1])
    # the symmetric state is the scalar ground state at g_eff = (g + g12) / 2, phi / sqrt(2) per component
    l, _, phi = gs._solve_on_grid([12.0], 1025, 8.0, 0.5, 0.5, 0)[12.0]
    assert np.abs(vs[:, 0] - phi / np.sqrt(2.0)).max() <= 1e-6 and abs(mf.chemical_potentials(vs, x, g)[0] - l) <= 1e-6 * l
    vp, Ep, _ = mf.flow(mf.start(x, norms, 1.0), x, g, norms)
    overlap = h * np.abs(vp[:, 0] * vp[:, 1]).sum() / 0.5
    assert Ep < Es - 0.03 and overlap < 0.8, (Es, Ep, overlap)      # (weakly immiscible: the components still share the wall)
    mu = mf.chemical_potentials(vp, x, g)
    r = [np.abs(_residual(vp, x, g, mu)[:, a]).max() for a in range(2)]
    assert max(r) <= 1e-5, r                                               # a stationary state, not a stalled flow


def _residual(v, x, g, mu):
    h = x[1] - x[0]
    vp = np.vstack([np.zeros((1, 2)), v, np.zeros((1, 2))])
    lap = (vp[2:] - 2.0 * vp[1:-1] + vp[:-2]) / (h * h)
    s = v * v
    nl = np.stack([g[0] * s[:, 0] + g[2] * s[:, 1], g[2] * s[:, 0] + g[1] * s[:, 1]], axis=1)
    return -0.5 * lap + (0.5 * x * x)[:, None] * v + nl * v - np.array(mu)[None, :] * v


def test_flow_energies_are_stable_under_grid_doubling():
    a = mf.sym_and_sep(n=513)
    b = mf.sym_and_sep(n=1025)
    print("E_sym, E_sep at n = 513:", a, " n = 1025:", b)
    assert abs(a[0] - b[0]) <= 1e-6 and abs(a[1] - b[1]) <= 1e-6
    assert b[1] < b[0]
