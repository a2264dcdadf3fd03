"""tests/mixture_observe_ref.py -- the fp64 reference tests/test_gpu_mixture_observe.py holds the mixture observables to -- held to what is
already pinned: its own sum rule, the energy of tests/mixture_energy_ref.py, two scalar records of tests/test_observables_cpu.py at
g_12 = 0, scale invariance, the two limits of the overlap -- and shown to tell a kernel without the cross coupling apart on the very
inputs of the GPU cells."""
import dataclasses

import numpy as np
import pytest

from oracle import gpe_oracle as go
from tests import mixture_cases as mc
from tests import mixture_energy_ref as mer
from tests import mixture_observe_ref as mo
from tests.test_observables_cpu import observables_ref

# one cell per forward family (tests/test_gpu_mixture_observe.py runs exactly these on the GPU)
CELLS = ("fused_2d_64x3_N37", "fused_2d_32x3_N1025", "fused_2d_128x2_N37", "padded_2d_72x3_N37", "wide_3d_256x2_N300",
         "generic_1d_48x2_N37", "generic_2d_64x2_N1025", "generic_3d_40_N37")
SCALARS = ("energy", "overlap", "res_rms_total")
PAIRS = ("kin", "pot", "mu", "mu_lap", "peak_density", "res_rms")

_REC = {}


def cell(name):
    """(mp, x, flat, U, V, fields, scale) of a GPU cell, computed once and left unchanged"""
    if name not in _REC:
        mp, x, flat, _, _, _ = mc.case(name)
        U, V = mo.jets(mp, flat, x)
        F, S = mo.record(U, x, V, mp.pb.kinetic_coeff, mp.g, mp.n, mp.pb.dx)
        _REC[name] = (mp, x, flat, U, V, F, S)
    return _REC[name]


@pytest.mark.parametrize("name", CELLS)
def test_sum_rule_and_the_energy_of_the_energy_term(name):
    mp, x, flat, U, V, F, _ = cell(name)
    lhs = sum(float(mp.n[a]) * F["mu"][a] for a in range(2))
    rhs = F["energy"] + sum(F["inter"])
    assert abs(lhs - rhs) <= 1e-12 * abs(rhs)
    assert F["energy"] == sum(F["kin"]) + sum(F["pot"]) + sum(F["inter"])
    E = mer.energy_of(mp, mer.local_sums(mp, flat, x))[0]               # dx = dv: the mixture energy term's own E
    assert abs(F["energy"] - E) <= 1e-12 * abs(E)
    assert abs(F["res_rms_total"] ** 2 - F["res_rms"][0] ** 2 - F["res_rms"][1] ** 2) <= 1e-12 * F["res_rms_total"] ** 2
    for a in range(2):                                                  # mu_lap: the kinetic part by parts
        assert F["mu_lap"][a] != F["mu"][a] and np.isfinite(F["mu_lap"][a])


@pytest.mark.parametrize("name", ["fused_2d_64x3_N37", "generic_1d_48x2_N37", "wide_3d_256x2_N300"])
def test_decoupled_components_are_two_scalar_records(name):
    """g_12 = 0: component a is the scalar problem with gamma = g_aa n_a on the network's output row a.  The scalar record describes
    u / sqrt(I) with norm 1, the mixture record sqrt(n_a) times that: mu_a = mu, the energy parts scale by n_a, res_rms by sqrt(n_a)."""
    mp, x, flat, U, V, _, _ = cell(name)
    g = (mp.g[0], mp.g[1], 0.0)
    F, _ = mo.record(U, x, V, mp.pb.kinetic_coeff, g, mp.n, mp.pb.dx)
    x64 = np.asarray(x, np.float64)
    E = 0.0
    for a in range(2):
        pb = dataclasses.replace(mp.pb, layers=list(mp.pb.layers[:-1]) + [1], gamma=g[a] * mp.n[a], p=3)
        f, _ = observables_ref(pb, x64, go.head_pde(pb, x64, U[:, :, a:a + 1] / pb.perturb_scale), pb.dx)
        na = float(mp.n[a])
        assert abs(F["mu"][a] - f["mu"]) <= 1e-12 * abs(f["mu"]) and abs(F["mu_lap"][a] - f["mu_lap"]) <= 1e-11 * abs(f["mu"])
        assert abs(F["norm"][a] - f["norm"]) <= 1e-13 * f["norm"]
        for k in ("kin", "pot", "inter"):
            assert abs(F[k][a] - na * f[k]) <= 1e-12 * abs(na * f[k]), (k, a)
        assert abs(F["res_rms"][a] - np.sqrt(na) * f["res_rms"]) <= 1e-11 * np.sqrt(na) * f["res_rms"]
        assert abs(F["peak_density"][a] - na * f["peak_density"]) <= 1e-12 * na * f["peak_density"]
        for k in range(3):
            assert abs(F["mean_x"][a][k] - f["mean_x"][k]) <= 1e-12 and abs(F["var_x"][a][k] - f["var_x"][k]) <= 1e-12
        E += na * f["energy"]
    assert F["inter"][2] == 0.0 and abs(F["energy"] - E) <= 1e-12 * abs(E)


def test_the_record_does_not_change_when_a_component_is_scaled():
    mp, x, flat, U, V, F, _ = cell("fused_2d_64x3_N37")
    lam = np.array([3.7, 0.21])
    G, _ = mo.record(U * lam[None, None, :], x, V, mp.pb.kinetic_coeff, mp.g, mp.n, mp.pb.dx)
    for a in range(2):
        assert abs(G["norm"][a] - lam[a] ** 2 * F["norm"][a]) <= 1e-13 * G["norm"][a]
    a, b = mo.flat(F), mo.flat(G)
    keep = np.ones(a.size, bool)
    keep[2:4] = False                                                    # norm[2]
    assert np.abs(a[keep] - b[keep]).max() <= 1e-11 * np.abs(a[keep]).max()
    assert np.all(np.abs(a[keep] - b[keep]) <= 1e-10 * np.maximum(np.abs(a[keep]), 1e-3))


def test_overlap_is_one_for_proportional_and_zero_for_disjoint_densities():
    mp, x, flat, U, V, F, _ = cell("generic_1d_48x2_N37")
    assert 0.0 < F["overlap"] < 1.0
    P = U.copy()
    P[:, :, 1] = 2.0 * P[:, :, 0]
    G, _ = mo.record(P, x, V, mp.pb.kinetic_coeff, mp.g, mp.n, mp.pb.dx)
    assert abs(G["overlap"] - 1.0) <= 1e-14
    D = U.copy()
    left = np.asarray(x)[:, 0] < 0.0
    D[:, left, 1] = 0.0
    D[:, ~left, 0] = 0.0
    G, _ = mo.record(D, x, V, mp.pb.kinetic_coeff, mp.g, mp.n, mp.pb.dx)
    assert G["overlap"] == 0.0 and G["inter"][2] == 0.0 and G["inter"][0] > 0.0 and G["inter"][1] > 0.0


@pytest.mark.parametrize("name", CELLS)
def test_the_gpu_cells_can_fail(name):
    """a chain that dropped the cross coupling (g_12 = 0) would move mu_1, mu_2 and the energy of every GPU cell by at least 1 %: far
    outside the 2e-5 those cells hold them to"""
    mp, x, flat, U, V, F, _ = cell(name)
    G, _ = mo.record(U, x, V, mp.pb.kinetic_coeff, (mp.g[0], mp.g[1], 0.0), mp.n, mp.pb.dx)
    for a in range(2):
        assert abs(G["mu"][a] - F["mu"][a]) >= 1e-2 * abs(F["mu"][a]), (name, a, G["mu"][a], F["mu"][a])
    assert abs(G["energy"] - F["energy"]) >= 1e-2 * abs(F["energy"]), (name, G["energy"], F["energy"])


def test_integer_weights_equal_the_repeated_points():
    mp, x, flat, U, V, _, _ = cell("fused_2d_64x3_N37")
    q = np.random.default_rng(2).integers(1, 4, x.shape[0])
    idx = np.repeat(np.arange(x.shape[0]), q)
    A, _ = mo.record(U, x, V, mp.pb.kinetic_coeff, mp.g, mp.n, mp.pb.dx, q=q)
    B, _ = mo.record(U[:, idx], np.asarray(x)[idx], V[idx], mp.pb.kinetic_coeff, mp.g, mp.n, mp.pb.dx)
    a, b = mo.flat(A), mo.flat(B)
    assert a[0] == x.shape[0] and b[0] == idx.size
    assert np.all(np.abs(a[1:] - b[1:]) <= 1e-11 * np.maximum(np.abs(b[1:]), 1e-3))
