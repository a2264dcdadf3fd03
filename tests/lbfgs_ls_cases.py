"""Analytic objectives and the case table shared by tests/test_gpu_lbfgs_ls.py (which injects them into the engine) and
tests/test_lbfgs_ls_reference_cpu.py (which asserts, on the CPU, that the reference's decisions on them keep their margins).
numpy only."""
import numpy as np

N = 256                                   # points of the GPU tests: an injected loss is float32(256 loss) / 256
SHAPE_PARAMS = {"P1153": 1153, "P12737": 12737, "P33537": 33537, "generic_P1153": 1153}
MARGIN_CAP = 1e-6


def start_params(P, seed=5):
    """tests/test_gpu_lbfgs.make_engine's parameters (its generator draws the N x d_in points first)"""
    d_in = 1 if P == 1153 else 2
    rng = np.random.default_rng(seed)
    rng.uniform(-3, 3, (N, d_in))
    return rng.normal(0, 0.3, P).astype(np.float32)


def representable(loss):
    return float(np.float32(loss * N)) / N


class Quadratic:
    """f = sum a (theta - star)^2 / 2, curvatures a in [0.5, 2], minimum 0"""
    def __init__(self, theta0, seed):
        rng = np.random.default_rng(seed)
        self.a = rng.uniform(0.5, 2.0, theta0.size)
        self.star = theta0.astype(np.float64) + rng.normal(0, 1.0, theta0.size)

    def __call__(self, theta):
        e = np.asarray(theta, np.float64) - self.star
        return 0.5 * float(np.sum(self.a * e * e)), self.a * e


class Rosenbrock:
    """paired Rosenbrock in shifted variables u = theta - shift: sum over pairs of 100 (u2 - u1^2)^2 + (1 - u1)^2 (an odd last element: a
    quadratic)"""
    def __init__(self, theta0, seed):
        rng = np.random.default_rng(seed)
        self.shift = theta0.astype(np.float64) - rng.uniform(-1.2, 1.2, theta0.size)
        self.n2 = theta0.size // 2 * 2

    def __call__(self, theta):
        u = np.asarray(theta, np.float64) - self.shift
        a, b = u[0:self.n2:2], u[1:self.n2:2]
        r = b - a * a
        g = np.zeros_like(u)
        g[0:self.n2:2] = -400.0 * a * r - 2.0 * (1.0 - a)
        g[1:self.n2:2] = 200.0 * r
        f = float(np.sum(100.0 * r * r + (1.0 - a) ** 2))
        if self.n2 < u.size:
            f += 0.5 * float(u[-1] ** 2)
            g[-1] = u[-1]
        return f, g


# objective, lr, objective seed (the first seeds at which the reference alone keeps every margin above 2e-6 on all shapes and both
# histories; most seeds of the quadratic do not: the cubic through a near-quadratic profile has a discriminant near 0): the tick-by-tick cells of the GPU test (each at history 3 and 10, on every shape)
TICK_CASES = {
    "quad_lr0.01": (Quadratic, 0.01, 4),
    "quad_lr8": (Quadratic, 8.0, 3),
    "rosen_lr1": (Rosenbrock, 1.0, 3),
}
TICKS = 14


def injected(obj, theta):
    """What the device is handed at theta: the fp32 gradient and a loss float32 can hold times 1/256"""
    f, g = obj(theta)
    return representable(f), g.astype(np.float32)


class LineProfile:
    """f(theta) = phi(u . (theta - theta_start)) with |u|_2 = 1: a 1-D profile under the first search (d = -phi'(0) u, so with
    phi'(0) = -1 the position along the line is the step t itself)"""
    def __init__(self, theta0, phi, dphi, seed=41):
        u = np.random.default_rng(seed).normal(0, 1, theta0.size)
        self.u = u / np.sqrt(u @ u)
        self.start = theta0.astype(np.float64)
        self.phi, self.dphi = phi, dphi

    def pos(self, theta):
        return float(self.u @ (np.asarray(theta, np.float64) - self.start))

    def __call__(self, theta):
        s = self.pos(theta)
        return self.phi(s), self.dphi(s) * self.u


def kink(s):
    return abs(s - 0.3) + 1.0


def dkink(s):
    return -1.0 if s < 0.3 else 1.0


# the ends of a search, one cell each: (phi, dphi, lr, settings of the configuration, the end the first search must take)
END_CELLS = {
    # ever steeper: the bracket phase extrapolates until max_ls = 3, then torch's fallback bracket [0, t]
    "max_ls": (lambda s: 4.0 - s - 0.05 * s * s, lambda s: -1.0 - 0.1 * s, 4.0, dict(max_ls=3), "end_max_ls"),
    # a kink: the curvature test never holds, the bracket shrinks until its width times max|d| is below tolerance_change
    "width": (kink, dkink, 30.0, dict(max_ls=60, tolerance_change=1e-2), "end_width"),
    # the same kink on a budget: ends by max_ls on the lower end of the bracket, which is not the trial evaluated last
    "not_last": (kink, dkink, 30.0, dict(max_ls=4), "end_max_ls"),
}
