"""Flat float64 restatement of torch.optim.LBFGS without a line search: the reference of the device-resident L-BFGS (csrc/gpe_lbfgs.h,
its state and freeze rule in csrc/gpe_lbfgs_rules.h).

torch's `opt.step(closure)` with max_iter = K evaluates the closure once per parameter update, in order.  Its `tolerance_change` and
`max_iter` breaks only end an outer call: the next call re-evaluates at the same parameters and carries on with the state it kept.  The
`gtd > -tolerance_change` break skips the update (direction, previous gradient and pairs are kept as formed).  So the optimiser is the flat
loop "evaluate (loss, g) at theta; iterate(loss, g)", and tests/test_lbfgs_reference_cpu.py holds this file to torch in fp64.

Rules beyond torch's, the engine's own: the state FREEZES for good once max|g| <= tolerance_grad (torch returns from every later call
before touching anything, as long as the objective is a function of theta), on a non-finite loss or gradient (torch has no such check),
or at loss < stop_loss when stop_loss > 0 (the drivers' stop).  A frozen iteration changes nothing, n_iter included.

ring_dtype = float32 restates the device's storage: the pair (s, y) = (t d, g - g_prev) is rounded to fp32 before its products are taken and
before it is stored, and d is kept in fp32; every product, sum and the recursion stay float64.  With float64 (default) it is torch in fp64.
No torch, no HIP."""
import numpy as np

LIVE, FROZEN_GRAD, FROZEN_NONFINITE, FROZEN_LOSS = 0, 1, 2, 3


class LbfgsRef:
    def __init__(self, theta, lr, history=100, tolerance_grad=1e-7, tolerance_change=1e-9, stop_loss=0.0, ring_dtype=np.float64):
        self.theta = np.asarray(theta, np.float64).copy()
        self.lr, self.history = float(lr), int(history)
        self.tolerance_grad, self.tolerance_change, self.stop_loss = float(tolerance_grad), float(tolerance_change), float(stop_loss)
        self.ring_dtype = np.dtype(ring_dtype)
        self.reset()

    def reset(self):
        self.S, self.Y, self.ro = [], [], []
        self.H_diag, self.t, self.n_iter, self.frozen = 1.0, 0.0, 0, LIVE
        self.d = np.zeros_like(self.theta)
        self.g_prev = np.zeros_like(self.theta)
        self.prev_loss = float("inf")

    def load(self, theta, S, Y, g_prev, d):
        """Take over parameters, pairs (oldest first), previous gradient and direction as a device holds them; ro follows from the pairs."""
        self.theta = np.asarray(theta, np.float64).copy()
        self.S = [np.asarray(s, np.float64) for s in S]
        self.Y = [np.asarray(y, np.float64) for y in Y]
        self.ro = [1.0 / float(y @ s) for s, y in zip(self.S, self.Y)]
        self.g_prev = np.asarray(g_prev, np.float64).copy()
        self.d = np.asarray(d, np.float64).copy()

    def iterate(self, loss, g):
        """One iteration on the evaluation (loss, g) at self.theta.  -> dict(status = 'applied' | 'skipped' | 'frozen', ...)."""
        rd = self.ring_dtype
        g = np.asarray(g, np.float64)
        loss = float(loss)
        gmax, g1 = (float(np.abs(g).max()), float(np.abs(g).sum())) if g.size else (0.0, 0.0)
        out = dict(loss=loss, grad_max=gmax, grad_l1=g1, pushed=0, ys=0.0)
        if not self.frozen:
            if not (np.isfinite(loss) and np.isfinite(g1)):
                self.frozen = FROZEN_NONFINITE
            elif gmax <= self.tolerance_grad:
                self.frozen = FROZEN_GRAD
            elif self.stop_loss > 0.0 and loss < self.stop_loss:
                self.frozen = FROZEN_LOSS
        if self.frozen:
            out.update(status="frozen", frozen=self.frozen, theta=self.theta.copy(), t=self.t, n_iter=self.n_iter, count=len(self.S), gtd=0.0)
            return out
        self.n_iter += 1
        if self.n_iter == 1:
            self.S, self.Y, self.ro, self.H_diag = [], [], [], 1.0
            d = -g
            cS, cY, cg = [], [], -1.0
        else:
            if rd == np.float32:
                y = (g.astype(np.float32) - self.g_prev.astype(np.float32)).astype(np.float64)
                s = (self.t * self.d).astype(np.float32).astype(np.float64)
            else:
                y, s = g - self.g_prev, self.t * self.d
            ys = float(y @ s)
            out["ys"] = ys
            if ys > 1e-10:
                if len(self.S) == self.history:
                    self.S.pop(0); self.Y.pop(0); self.ro.pop(0)
                self.S.append(s); self.Y.append(y); self.ro.append(1.0 / ys)
                self.H_diag = ys / float(y @ y)
                out["pushed"] = 1
            n = len(self.S)
            al = [0.0] * n
            q = -g
            for i in range(n - 1, -1, -1):
                al[i] = float(self.S[i] @ q) * self.ro[i]
                q = q - al[i] * self.Y[i]
            d = q * self.H_diag
            cS = [0.0] * n
            for i in range(n):
                be = float(self.Y[i] @ d) * self.ro[i]
                cS[i] = al[i] - be
                d = d + cS[i] * self.S[i]
            cY, cg = [-self.H_diag * a for a in al], -self.H_diag
        # sum_j |c_j b_j| per element: what an error of the coefficients multiplies (the bound of tests/test_gpu_lbfgs.py)
        absum = np.abs(cg * g)
        for c, b in list(zip(cS, self.S)) + list(zip(cY, self.Y)):
            absum = absum + np.abs(c * b)
        self.g_prev = g.copy()
        self.prev_loss = loss
        self.t = min(1.0, 1.0 / g1) * self.lr if self.n_iter == 1 else self.lr
        gtd = float(g @ d)
        self.d = d.astype(np.float32).astype(np.float64) if rd == np.float32 else d
        out.update(frozen=LIVE, t=self.t, n_iter=self.n_iter, count=len(self.S), gtd=gtd, d=d, absum=absum, H_diag=self.H_diag)
        if gtd > -self.tolerance_change:
            out.update(status="skipped", theta=self.theta.copy())
            return out
        self.theta = self.theta + self.t * self.d
        out.update(status="applied", theta=self.theta.copy())
        return out


def run_flat(ref, fun, n_iters):
    """n_iters times "evaluate, iterate" on fun(theta) -> (loss, g); -> list of the iterations' dicts."""
    outs = []
    for _ in range(n_iters):
        loss, g = fun(ref.theta)
        outs.append(ref.iterate(loss, g))
    return outs


def direction_from_gram(S, Y, g, H_diag):
    """The device's form of the two-loop recursion (csrc/gpe_lbfgs.h): coefficients of d over {S_j, Y_j, g} from the dot-product blocks
    S.Y, Y.Y and the row of g alone.  S, Y: pairs oldest first.  -> (cS, cY, cg, g.d); d = sum cS_j S_j + sum cY_j Y_j + cg g."""
    n = len(S)
    g = np.asarray(g, np.float64)
    if n == 0:
        return np.zeros(0), np.zeros(0), -H_diag, -H_diag * float(g @ g)
    Sm, Ym = np.asarray(S, np.float64), np.asarray(Y, np.float64)
    SY, YY, Sg, Yg = Sm @ Ym.T, Ym @ Ym.T, Sm @ g, Ym @ g
    ro = 1.0 / np.diag(SY)
    al, cS = np.zeros(n), np.zeros(n)
    w = -Sg.copy()
    for i in range(n - 1, -1, -1):
        al[i] = ro[i] * w[i]
        w[:i] -= al[i] * SY[:i, i]
    v = H_diag * (-Yg - YY @ al)
    for i in range(n):
        cS[i] = al[i] - ro[i] * v[i]
        v[i + 1:] += cS[i] * SY[i, i + 1:]
    cY = -H_diag * al
    return cS, cY, -H_diag, float(-H_diag * (g @ g) + cS @ Sg + cY @ Yg)
