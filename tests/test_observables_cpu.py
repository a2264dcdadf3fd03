"""CPU side of the device observables (include/gpe_hip.h: struct gpe_observables): the four entry points are declared and exported,
the ctypes struct has the library's size, and the fp64 reference that tests/test_gpu_observables.py holds the kernels to --
observables_ref(), from oracle.gpe_oracle.head_pde output -- reproduces closed forms."""
import ctypes
import math
import os
import re

import numpy as np

from gpe_pinn import capi
from oracle import gpe_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gpe_sizeof_observables", "gpe_observables", "gpe_bind_monitor", "gpe_read_monitor")


def observables_ref(pb, x, hp, dv):
    """fp64 reference of struct gpe_observables from head_pde(pb, x, jets) = dict(U [C,N,out], Hu [N,out], V [N]) on the points x [N,d].
    -> (fields, scale): scale[k] = dv * sum |summand| (normalised like the field) for the fields whose sums cancel (lz, rot, mean_x,
    var_x), plus res_field_max = max |H[phi] phi - mu phi| for the bound on res_rms."""
    U, Hu, V = (np.asarray(hp[k], np.float64) for k in ("U", "Hu", "V"))
    x = np.asarray(x, np.float64)
    N, d = x.shape
    p = 3 if pb.complex_psi else int(pb.p)
    c, Om = float(pb.kinetic_coeff), float(pb.omega_rot)
    u = U[0]
    rho = (u * u).sum(axis=1)
    lap = U[1 + d:1 + 2 * d].sum(axis=0)
    lin = -c * lap + V[:, None] * u                                   # linear part of H u
    lz_s = np.zeros(N)
    if pb.complex_psi and d >= 2:
        Dr = x[:, 0] * U[2, :, 0] - x[:, 1] * U[1, :, 0]              # (x d_y - y d_x) psi_r
        Di = x[:, 0] * U[2, :, 1] - x[:, 1] * U[1, :, 1]
        lz_s = u[:, 0] * Di - u[:, 1] * Dr
        if Om != 0.0:
            lin = lin + np.stack([-Om * Di, Om * Dr], axis=1)         # -Omega L_z psi = i Omega (x d_y - y d_x) psi
    non = Hu - lin                                                    # the oracle's own nonlinear term N(u)
    sr = rho.sum()
    I = dv * sr
    f = dict(n=float(N), dv=float(dv), norm=I)
    f["kin"] = c * (U[1:1 + d] ** 2).sum() / sr
    f["pot"] = (V * rho).sum() / sr
    f["inter"] = 2.0 / (p + 1) * dv * (u * non).sum() / I ** (0.5 * (p + 1))
    f["lz"] = lz_s.sum() / sr
    f["rot"] = -Om * f["lz"]
    f["energy"] = f["kin"] + f["pot"] + f["inter"] + f["rot"]
    tail = f["pot"] + 0.5 * (p + 1) * f["inter"] + f["rot"]
    f["mu"] = f["kin"] + tail
    f["mu_lap"] = -c * (u * lap).sum() / sr + tail
    xs = np.concatenate([x, np.zeros((N, 3 - d))], axis=1)
    m1 = (xs * rho[:, None]).sum(axis=0) / sr
    m2 = (xs * xs * rho[:, None]).sum(axis=0) / sr
    a1 = (np.abs(xs) * rho[:, None]).sum(axis=0) / sr
    f["mean_x"] = list(m1)
    f["var_x"] = list(m2 - m1 * m1)
    f["peak_density"] = rho.max() / I
    r = (lin - f["mu"] * u) / math.sqrt(I) + non / I ** (0.5 * p)     # H[phi] phi - mu phi, phi = u / sqrt(I)
    f["res_rms"] = math.sqrt(dv * (r * r).sum())
    la = np.abs(lz_s).sum() / sr
    # var_x = m2 - m1^2: an error e2 of m2 and e1 of m1 move it by e2 + 2 |m1| e1
    scale = dict(lz=la, rot=abs(Om) * la, mean_x=list(a1), var_x=list(m2 + 2.0 * np.abs(m1) * a1), res_field_max=float(np.abs(r).max()))
    return f, scale


def _header():
    txt = open(os.path.join(ROOT, "include", "gpe_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_and_library_exports_the_entry_points():
    txt = _header()
    lib = ctypes.CDLL(capi.library_path())
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} not declared in include/gpe_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in capi.SYMBOLS
    assert re.search(r"struct\s+gpe_observables\s*\{", txt)


def test_struct_size_matches_the_library():
    lib = ctypes.CDLL(capi.library_path())
    lib.gpe_sizeof_observables.restype = ctypes.c_size_t
    assert lib.gpe_sizeof_observables() == ctypes.sizeof(capi.gpe_observables) == 20 * 8
    d = capi.gpe_observables().as_dict()
    assert list(d)[:4] == ["n", "dv", "step", "norm"] and len(d["mean_x"]) == 3 and len(d["var_x"]) == 3


def test_reference_1d_harmonic_ground_state_closed_forms():
    """exp(-x^2/2) with c = 1, V = x^2, g = 0, fed as exact jets: E = mu = mu_lap = 1 (kin = pot = 1/2), var_x = 1/2, residual 0."""
    x = np.linspace(-12.0, 12.0, 4801).reshape(-1, 1)
    dv = float(x[1, 0] - x[0, 0])
    g = 0.7 * np.exp(-0.5 * x[:, 0] ** 2)                              # unnormalised on purpose: the struct describes u / sqrt(I)
    jets = np.stack([g, -x[:, 0] * g, (x[:, 0] ** 2 - 1.0) * g])[:, :, None]
    pb = go.Problem(layers=[1, 8, 1], kinetic_coeff=1.0, pot_scale=1.0, gamma=0.0, dx=dv)
    f, s = observables_ref(pb, x, go.head_pde(pb, x, jets), dv)
    assert abs(f["norm"] - 0.49 * math.sqrt(math.pi)) < 1e-10
    for k, v in (("kin", 0.5), ("pot", 0.5), ("inter", 0.0), ("rot", 0.0), ("energy", 1.0), ("mu", 1.0), ("mu_lap", 1.0), ("lz", 0.0)):
        assert abs(f[k] - v) < 1e-10, (k, f[k])
    assert abs(f["mean_x"][0]) < 1e-10 and abs(f["var_x"][0] - 0.5) < 1e-10 and f["var_x"][1:] == [0.0, 0.0]
    assert abs(f["peak_density"] - 1.0 / math.sqrt(math.pi)) < 1e-10
    assert f["res_rms"] < 1e-10 and s["res_field_max"] < 1e-10


def test_reference_1d_interaction_scaling():
    """g > 0, p = 3: inter = g/2 int phi^4 for the normalised Gaussian phi, = g / (2 sqrt(2 pi)); mu - E = inter."""
    x = np.linspace(-12.0, 12.0, 4801).reshape(-1, 1)
    dv = float(x[1, 0] - x[0, 0])
    g = 1.9 * np.exp(-0.5 * x[:, 0] ** 2)
    jets = np.stack([g, -x[:, 0] * g, (x[:, 0] ** 2 - 1.0) * g])[:, :, None]
    pb = go.Problem(layers=[1, 8, 1], kinetic_coeff=0.5, pot_scale=0.5, gamma=3.0, dx=dv)
    f, _ = observables_ref(pb, x, go.head_pde(pb, x, jets), dv)
    assert abs(f["inter"] - 3.0 / (2.0 * math.sqrt(2.0 * math.pi))) < 1e-10
    assert abs(f["mu"] - f["energy"] - f["inter"]) < 1e-12 and abs(f["kin"] - 0.25) < 1e-10 and abs(f["pot"] - 0.25) < 1e-10


def test_reference_2d_vortex_state_has_unit_angular_momentum():
    """(x + i y) exp(-r^2/2): <L_z> = 1; with c = 1/2, V = r^2/2, g = 0 it is an eigenstate with mu = 2, rotating frame mu = 2 - Omega."""
    ax = np.linspace(-9.0, 9.0, 361)
    X, Y = np.meshgrid(ax, ax, indexing="ij")
    x = np.stack([X.ravel(), Y.ravel()], axis=1)
    dv = float(ax[1] - ax[0]) ** 2
    xx, yy = x[:, 0], x[:, 1]
    w = np.exp(-0.5 * (xx * xx + yy * yy))

    def jets_of(f0, fx, fy, fxx, fyy):        # f = poly * w, poly in {x, y}
        return np.stack([f0 * w, fx * w, fy * w, fxx * w, fyy * w])

    re_ = jets_of(xx, 1 - xx * xx, -xx * yy, xx ** 3 - 3 * xx, xx * (yy * yy - 1))
    im_ = jets_of(yy, -xx * yy, 1 - yy * yy, yy * (xx * xx - 1), yy ** 3 - 3 * yy)
    jets = np.stack([re_, im_], axis=2)
    Om = 0.3
    pb = go.Problem(layers=[2, 8, 2], complex_psi=True, kinetic_coeff=0.5, pot_scale=0.5, gamma=0.0, omega_rot=Om, dx=dv)
    f, s = observables_ref(pb, x, go.head_pde(pb, x, jets), dv)
    assert abs(f["lz"] - 1.0) < 1e-10 and abs(f["rot"] + Om) < 1e-10
    assert abs(f["mu"] - (2.0 - Om)) < 1e-10 and abs(f["mu_lap"] - (2.0 - Om)) < 1e-10 and abs(f["energy"] - (2.0 - Om)) < 1e-10
    assert abs(f["norm"] - math.pi) < 1e-9 and f["res_rms"] < 1e-9
    assert abs(f["var_x"][0] - 1.0) < 1e-10 and abs(f["var_x"][1] - 1.0) < 1e-10 and abs(f["mean_x"][0]) < 1e-10
    assert abs(s["lz"] - 1.0) < 1e-10          # the summand rho is positive here: nothing cancels
