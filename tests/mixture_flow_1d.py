"""Normalised gradient flow for two REAL components on a 1D grid, fp64 numpy / scipy.  TEST INFRASTRUCTURE, not product: the yardstick for
the energies a trained mixture is judged by (tests/test_gpu_mixture_energy.py, tools/accuracy_mixture.py).

  E[v] = sum_a int (c v_a'^2 + V v_a^2) + 1/2 sum_ab g_ab int v_a^2 v_b^2 ,   int v_a^2 = n_a ,   V = vscale x^2

Second-order finite differences on [-half, half] with v = 0 at the ends; one step is backward Euler on the operator frozen at the current
state, (1 + dt H_a[v]) w_a = v_a, then w_a is scaled back to norm n_a (Bao & Du's BEFD scheme): unconditionally stable, the energy
decreases, and its fixed points are the solutions of H_a v_a = mu_a v_a.  A start with v_1 = v_2 (equal n_a, g_11 = g_22) stays so,
bit for bit -- both components see the same arithmetic -- and ends on the symmetric stationary state whatever g_12 is; a start with the
components apart ends on the separated state when g_12^2 > g_11 g_22.  energy() is second order in h; energies come Richardson-extrapolated
from grids n and 2n - 1 (richardson_energy)."""
import numpy as np
from scipy.linalg import solve_banded


def grid(n, half):
    x = np.linspace(-half, half, n)
    return x, x[1] - x[0]


def energy(v, x, g, c=0.5, vscale=0.5):
    """E of the state v [n, 2] as it is (no normalisation): trapezoid = h * sum with v = 0 at the ends; the kinetic term on the half points"""
    h = x[1] - x[0]
    V = vscale * x * x
    dv = np.diff(np.vstack([np.zeros((1, 2)), v, np.zeros((1, 2))]), axis=0) / h
    s = v * v
    g11, g22, g12 = g
    return float(h * (c * (dv * dv).sum() + (V[:, None] * s).sum()
                      + 0.5 * g11 * (s[:, 0] ** 2).sum() + 0.5 * g22 * (s[:, 1] ** 2).sum() + g12 * (s[:, 0] * s[:, 1]).sum()))


def chemical_potentials(v, x, g, c=0.5, vscale=0.5):
    h = x[1] - x[0]
    V = vscale * x * x
    vp = np.vstack([np.zeros((1, 2)), v, np.zeros((1, 2))])
    lap = (vp[2:] - 2.0 * vp[1:-1] + vp[:-2]) / (h * h)
    s = v * v
    g11, g22, g12 = g
    Hv = -c * lap + V[:, None] * v + np.stack([g11 * s[:, 0] + g12 * s[:, 1], g12 * s[:, 0] + g22 * s[:, 1]], axis=1) * v
    return tuple(float((v[:, a] * Hv[:, a]).sum() / (v[:, a] ** 2).sum()) for a in range(2))


def flow(v0, x, g, norms, c=0.5, vscale=0.5, dt=0.05, tol=1e-13, max_steps=20000):
    """-> (v [n, 2], E, steps): iterate until the energy moves by less than tol (absolute) in a step"""
    h = x[1] - x[0]
    n = x.size
    V = vscale * x * x
    g11, g22, g12 = g
    v = np.array(v0, np.float64)
    for a in range(2):
        v[:, a] *= np.sqrt(norms[a] / (h * (v[:, a] ** 2).sum()))
    off = np.full(n, -dt * c / (h * h))
    E = energy(v, x, g, c, vscale)
    for k in range(max_steps):
        s = v * v
        nl = (g11 * s[:, 0] + g12 * s[:, 1], g12 * s[:, 0] + g22 * s[:, 1])
        w = np.empty_like(v)
        for a in range(2):
            ab = np.vstack([off, 1.0 + dt * (2.0 * c / (h * h) + V + nl[a]), off])
            w[:, a] = solve_banded((1, 1), ab, v[:, a])
            w[:, a] *= np.sqrt(norms[a] / (h * (w[:, a] ** 2).sum()))
        v = w
        E_new = energy(v, x, g, c, vscale)
        done = abs(E_new - E) < tol
        E = E_new
        if done:
            break
    return v, E, k + 1


def start(x, norms, shift):
    """Gaussians of the linear problem, component 1 displaced by -shift and component 2 by +shift (shift = 0: v_1 / sqrt(n_1) = v_2 / sqrt(n_2))"""
    return np.stack([np.sqrt(norms[0]) * np.exp(-0.5 * (x + shift) ** 2), np.sqrt(norms[1]) * np.exp(-0.5 * (x - shift) ** 2)], axis=1)


def stationary_energy(g, norms, shift, n=1025, half=8.0, c=0.5, vscale=0.5, **kw):
    """E of the state the flow ends on from start(shift), on the grid of n points"""
    x, _ = grid(n, half)
    return flow(start(x, norms, shift), x, g, norms, c, vscale, **kw)[1]


def richardson_energy(g, norms, shift, n=1025, half=8.0, **kw):
    """(4 E(2n - 1) - E(n)) / 3: the h^2 term of the second-order scheme removed"""
    return (4.0 * stationary_energy(g, norms, shift, 2 * n - 1, half, **kw) - stationary_energy(g, norms, shift, n, half, **kw)) / 3.0


_CACHE = {}


def sym_and_sep(g=10.0, g12=14.0, n=1025, half=8.0):
    """(E_sym, E_sep) of the immiscible DESIGN case: g_11 = g_22 = g, n_a = 1/2, V = x^2 / 2, c = 1/2 -- the symmetric stationary state
    (start with v_1 = v_2) and the separated one (components started one trap length apart).  Computed once per process."""
    key = (g, g12, n, half)
    if key not in _CACHE:
        G, norms = (g, g, g12), (0.5, 0.5)
        _CACHE[key] = (richardson_energy(G, norms, 0.0, n, half), richardson_energy(G, norms, 1.0, n, half))
    return _CACHE[key]
