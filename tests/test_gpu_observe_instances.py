"""Every instance of the observables chain (csrc/gpe_observe.h: 2 kinds x 3 dims x weighted or not) against fp64 host sums over the
engine's own jets: the same fp64 products of the same fp32 numbers (the potential is a precomputed fp32 array), only the order of addition
differs.  Every field of the record is held.

The cells (tests/observe_cells.py): scalar real and mixture in 1, 2, 3 dimensions, scalar complex with rotation in 2 and 3; no weights
(an explicit set) and real positive weights (the bound set); N = 1 (one thread), 257 (one workgroup and one point) and 262 149 =
OBS_MAX_WG * OBS_THREADS + 5 (threads loop).  The tolerance is the one of
  tests/test_gpu_observables.py::test_observables_equal_fp64_host_sums_over_the_engines_own_jets
  tests/test_gpu_weights.py::test_observables_with_real_weights_equal_fp64_host_sums_over_the_engines_own_jets
  tests/test_gpu_mixture_observe.py::test_equals_fp64_host_sums_over_the_engines_own_jets
-- 1e-9 relative to sum |summand| (N 2^-53 = 3e-11 at these sizes), res_rms relative to itself as the mixture test holds it."""
import numpy as np
import pytest

from tests import mixture_observe_ref as mo
from tests import observe_cells as oc
from tests.test_gpu_mixture_observe import _hold_to_host_sums, hold

pytestmark = pytest.mark.gpu

TOL = 1e-9


def scalar_record(pb, J, x, V, dv, q):
    """struct gpe_observables from the jets J [C][N][n_out] by the formulas of include/gpe_hip.h, in fp64 with the engine's fp32
    constants; and the sum of |summand| behind every field, normalised like the field"""
    N, d = x.shape
    f32 = lambda v: float(np.float32(v))
    c, g, Om, dv = f32(pb.kinetic_coeff), f32(pb.gamma), f32(pb.omega_rot), f32(dv)
    x64, V64 = x.astype(np.float64), V.astype(np.float64)
    w = np.ones(N) if q is None else q
    u, gr, lap = J[0], J[1:1 + d], J[1 + d:1 + 2 * d].sum(axis=0)
    rho = (u * u).sum(axis=1)
    sr = (w * rho).sum()
    I = dv * sr
    p = 3 if pb.complex_psi else pb.p
    s = g * rho * rho if pb.complex_psi else g * u[:, 0] ** (p - 1) * u[:, 0] * u[:, 0]
    zero = np.zeros(N)
    Dr, Di = (x64[:, 0] * gr[1, :, 0] - x64[:, 1] * gr[0, :, 0], x64[:, 0] * gr[1, :, 1] - x64[:, 1] * gr[0, :, 1]) if pb.complex_psi else (zero, zero)
    lz_s = u[:, 0] * Di - u[:, 1] * Dr if pb.complex_psi else zero
    ulap = (u * lap).sum(axis=1)
    ipow = I ** (0.5 * (p + 1))
    r = dict(norm=I, kin=c * (w * (gr ** 2).sum(axis=(0, 2))).sum() / sr, pot=(w * V64 * rho).sum() / sr,
             inter=2.0 / (p + 1) * dv * (w * s).sum() / ipow, lz=(w * lz_s).sum() / sr)
    a = dict(inter=2.0 / (p + 1) * dv * (w * np.abs(s)).sum() / ipow, lz=(w * np.abs(lz_s)).sum() / sr)
    r["rot"] = -Om * r["lz"]
    a["rot"] = abs(Om) * a["lz"]
    r["energy"] = r["kin"] + r["pot"] + r["inter"] + r["rot"]
    a["energy"] = r["kin"] + r["pot"] + a["inter"] + a["rot"]
    tail, atail = r["pot"] + 0.5 * (p + 1) * r["inter"] + r["rot"], r["pot"] + 0.5 * (p + 1) * a["inter"] + a["rot"]
    r["mu"], a["mu"] = r["kin"] + tail, r["kin"] + atail
    r["mu_lap"], a["mu_lap"] = -c * (w * ulap).sum() / sr + tail, c * (w * np.abs(ulap)).sum() / sr + atail
    r["mean_x"], r["var_x"], a["mean_x"], a["var_x"] = [0.0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3
    for k in range(d):
        m1, m2, a1 = (w * x64[:, k] * rho).sum() / sr, (w * x64[:, k] ** 2 * rho).sum() / sr, (w * np.abs(x64[:, k]) * rho).sum() / sr
        r["mean_x"][k], r["var_x"][k], a["mean_x"][k], a["var_x"][k] = m1, m2 - m1 * m1, a1, m2 + 2 * abs(m1) * a1
    r["peak_density"] = rho.max() / I                       # the plain maximum, weights or not
    # H[phi] phi - mu phi, phi = u / sqrt(I): linear part and nonlinear term per component
    lin = -c * lap + V64[:, None] * u
    if pb.complex_psi:
        lin = lin + np.stack([-Om * Di, Om * Dr], axis=1)
        non = g * rho[:, None] * u
    else:
        non = g * u ** (p - 1) * u
    res = (lin - r["mu"] * u) / np.sqrt(I) + non * I ** (-0.5 * p)
    r["res_rms"] = float(np.sqrt(dv * (w * (res * res).sum(axis=1)).sum()))
    return r, a


@pytest.mark.parametrize("N", oc.SIZES)
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", list(oc.SCALAR))
def test_scalar_instances_equal_fp64_host_sums_over_the_engines_own_jets(name, weighted, N):
    pb, x, V, dv, J, q, got = oc.scalar_cell(name, N, weighted)
    ref, scale = scalar_record(pb, J, x, V, dv, q)
    d = x.shape[1]
    assert got["n"] == N and got["step"] == 0.0 and abs(got["dv"] - dv) <= 1e-7 * dv
    rows = [(k, got[k], ref[k], TOL * abs(ref[k])) for k in ("norm", "kin", "pot", "peak_density", "res_rms")]
    rows += [(k, got[k], ref[k], TOL * scale[k]) for k in ("inter", "lz", "rot", "energy", "mu", "mu_lap")]
    rows += [(f"{k}[{j}]", got[k][j], ref[k][j], TOL * scale[k][j]) for k in ("mean_x", "var_x") for j in range(d)]
    hold(rows)
    assert all(got[k][j] == 0.0 for k in ("mean_x", "var_x") for j in range(d, 3))         # the unused axes
    if not pb.complex_psi:
        assert got["lz"] == 0.0 and got["rot"] == 0.0


@pytest.mark.parametrize("N", oc.SIZES)
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_mixture_instances_equal_fp64_host_sums_over_the_engines_own_jets(d, weighted, N):
    mp, x, V, dv, J, q, got = oc.mixture_cell(d, N, weighted)
    f32 = lambda v: [float(np.float32(t)) for t in v]
    ref, scale = mo.record(J, x.astype(np.float64), V.astype(np.float64), float(np.float32(mp.pb.kinetic_coeff)), f32(mp.g), f32(mp.n),
                           float(np.float32(dv)), q=q)
    assert got["n"] == N
    _hold_to_host_sums(got, ref, scale, dim=d)
