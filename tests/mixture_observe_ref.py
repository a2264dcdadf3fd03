"""fp64 reference of struct gpe_mixture_observables (include/gpe_hip.h) from the jets of the two components.

  record(U, x, V, c, g, n, dv, q=None) -> (fields, scale)

U [C, N, 2], C = 1 + 2 d: the u-jets of both components (value, d first, d diagonal second derivatives; perturb_scale included), x [N, d],
V [N], c = kinetic_coeff, g = (g11, g22, g12), n = (n_1, n_2) the target norms, dv the quadrature weight, q optional per-point weights.
Everything but `norm` describes the state normalised to the target norms, v_a = u_a sqrt(n_a / I_a), and is written here ON v_a -- not
through the quotients of raw sums the header states and the kernel forms -- so the two derivations check each other.
scale: sum |summand| (normalised like the field) for the fields whose sums cancel (mu_lap's kinetic part, mean_x, var_x), and
res_field_max[a] = max |H_a[v] v_a - mu_a v_a| for the bound on res_rms[a]."""
import math

import numpy as np

from oracle import gpe_oracle as go


def jets(mp, flat, x):
    """(U [C, N, 2], V [N]) of the oracle's network for the MixProblem mp (tests/mixture_ref.py) on the points x, in fp64"""
    pb = mp.pb
    x = np.asarray(x, np.float64)
    out, _ = go.mlp_forward(go.unflatten(np.asarray(flat, np.float64), pb.layers), x, pb.activation)
    return pb.perturb_scale * out, go.potential(pb, x)


def record(U, x, V, c, g, n, dv, q=None):
    U, x, V = np.asarray(U, np.float64), np.asarray(x, np.float64), np.asarray(V, np.float64)
    N, d = x.shape
    q = np.ones(N) if q is None else np.asarray(q, np.float64).ravel()
    g11, g22, g12 = (float(v) for v in g)
    G = np.array([[g11, g12], [g12, g22]])
    nt = np.array([float(n[0]), float(n[1])])
    c, dv = float(c), float(dv)
    u = U[0]
    I = dv * (q[:, None] * u * u).sum(axis=0)                              # raw norms
    f = np.sqrt(nt / I)
    v, dvk, lap = f * u, f * U[1:1 + d], f * U[1 + d:1 + 2 * d].sum(axis=0)  # the normalised state and its derivatives
    w = q * dv                                                             # the measure
    rho = v * v
    F = dict(n=float(N), dv=dv, norm=list(I))
    F["kin"] = [float(c * (w[:, None] * (dvk * dvk).sum(axis=0))[:, a].sum()) for a in range(2)]
    F["pot"] = [float((w * V * rho[:, a]).sum()) for a in range(2)]
    F["inter"] = [float(0.5 * g11 * (w * rho[:, 0] ** 2).sum()), float(0.5 * g22 * (w * rho[:, 1] ** 2).sum()),
                  float(g12 * (w * rho[:, 0] * rho[:, 1]).sum())]
    F["energy"] = sum(F["kin"]) + sum(F["pot"]) + sum(F["inter"])
    Hv = -c * lap + V[:, None] * v + (rho @ G.T) * v                       # H_a[v] v_a
    mu, mu_lap, lap_abs = [], [], []
    for a in range(2):
        tail = F["pot"][a] + (w * (rho @ G.T)[:, a] * rho[:, a]).sum()
        mu.append(float((F["kin"][a] + tail) / nt[a]))
        mu_lap.append(float(((w * v[:, a] * (-c * lap[:, a])).sum() + tail) / nt[a]))
        lap_abs.append(float((w * np.abs(v[:, a] * c * lap[:, a])).sum() / nt[a]))
    F["mu"], F["mu_lap"] = mu, mu_lap
    q11, q22, q12 = (w * rho[:, 0] ** 2).sum(), (w * rho[:, 1] ** 2).sum(), (w * rho[:, 0] * rho[:, 1]).sum()
    F["overlap"] = float(q12 / math.sqrt(q11 * q22)) if q11 > 0 and q22 > 0 else float("nan")
    xs = np.concatenate([x, np.zeros((N, 3 - d))], axis=1)
    m1 = np.stack([(w[:, None] * xs * rho[:, a:a + 1]).sum(axis=0) / nt[a] for a in range(2)])
    m2 = np.stack([(w[:, None] * xs * xs * rho[:, a:a + 1]).sum(axis=0) / nt[a] for a in range(2)])
    a1 = np.stack([(w[:, None] * np.abs(xs) * rho[:, a:a + 1]).sum(axis=0) / nt[a] for a in range(2)])
    F["mean_x"] = [list(r) for r in m1]
    F["var_x"] = [list(r) for r in m2 - m1 * m1]
    F["peak_density"] = [float(rho[:, a].max()) for a in range(2)]
    r = Hv - np.array(mu)[None, :] * v
    F["res_rms"] = [float(math.sqrt((w * r[:, a] ** 2).sum())) for a in range(2)]
    F["res_rms_total"] = math.sqrt(F["res_rms"][0] ** 2 + F["res_rms"][1] ** 2)
    # var_x = m2 - m1^2: an error e2 of m2 and e1 of m1 move it by e2 + 2 |m1| e1 (tests/test_observables_cpu.py)
    scale = dict(mu_lap=lap_abs, mean_x=[list(r) for r in a1], var_x=[list(r) for r in m2 + 2.0 * np.abs(m1) * a1],
                 res_field_max=[float(np.abs(r[:, a]).max()) for a in range(2)])
    return F, scale


def flat(F):
    """the record's numbers in the struct's order (without step), as Engine.MIXTURE_OBSERVABLE_FIELDS names them"""
    out = [F["n"], F["dv"]]
    for k in ("norm", "kin", "pot", "inter"):
        out += list(F[k])
    out.append(F["energy"])
    for k in ("mu", "mu_lap"):
        out += list(F[k])
    out.append(F["overlap"])
    for k in ("mean_x", "var_x"):
        out += [v for r in F[k] for v in r]
    for k in ("peak_density", "res_rms"):
        out += list(F[k])
    out.append(F["res_rms_total"])
    return np.array(out, np.float64)
