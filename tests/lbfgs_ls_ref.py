"""Flat float64 restatement of torch.optim.LBFGS with line_search_fn = "strong_wolfe": the reference of the device-resident line search
(csrc/gpe_lbfgs_rules.h: ls_decide, ls_rearm; csrc/gpe_lbfgs.h: k_ls_dots, k_ls_decide and the LS instantiations of the three iteration
kernels).

torch's `_strong_wolfe` is a loop that calls the objective where it needs a value.  Here it is a state machine that CONSUMES one evaluation
per call: tick(loss, g) takes the evaluation at the current point self.theta (= theta0 + t d, or theta0 itself when no search is running)
and either names the next trial step or accepts a point of the bracket.  An accepted point hands its STORED loss and gradient to
lbfgs_ref.LbfgsRef.iterate (imported, not copied), which forms the next direction; no new evaluation happens in between, as in torch.
tests/test_lbfgs_ls_reference_cpu.py holds this file to torch in fp64.

States (what the next evaluation is for): IDLE (it is taken at theta0: the very first one, or the one after a g.d > -tolerance_change
skip), BRACKET, ZOOM.  In BRACKET the previous trial lives in bracket end 0 (t_prev = b[0]); forming torch's bracket [t_prev, t] fills
end 1.  Gradients live in slots 0..2 referred to by index (slot 3 = the start gradient, LbfgsRef.g_prev); none is ever copied.

Rules beyond torch's, the engine's own: the freezes of lbfgs_ref.py at an accepted point; a non-finite loss or gradient AT A TRIAL puts
theta back to the best point the bracket holds (t_low in ZOOM, 0 in BRACKET) and freezes with code 2; `stalled` counts accepted steps
with t = 0 (theta unchanged, no pair pushed); torch's lack-of-progress breaks only end an outer call and are not restated.

Every comparison a decision rests on records its relative margin in self.margins (reset per tick): two sides that differ by less than
the margin could decide otherwise under a rounding error of that size.  Comparisons of two stored losses are exact on both sides when
the losses are the same numbers, and record no margin when they are equal.  exact_losses = True says that whoever is compared with
this machine is fed the very same loss values (the GPU tests' injection): the Armijo test's margin is then taken relative to
c1 t g0.d, the only term of it that can differ, not to the loss.

ring_dtype = float32 restates the device's storage as lbfgs_ref.py does; in addition every point is fl32(theta0 + t d), formed in fp64 and
rounded once.  No torch, no HIP."""
import numpy as np

from tests.lbfgs_ref import LbfgsRef, FROZEN_NONFINITE

IDLE, BRACKET, ZOOM = 0, 1, 2
PHASES = ("none", "bracket", "zoom", "accepted", "frozen")          # what a tick did: the record's `phase` is the index
START_SLOT = 3


class LbfgsLsRef:
    def __init__(self, theta, lr, history=100, tolerance_grad=1e-7, tolerance_change=1e-9, stop_loss=0.0, c1=1e-4, c2=0.9, max_ls=25,
                 ring_dtype=np.float64, exact_losses=False):
        self.exact_losses = bool(exact_losses)
        self.lb = LbfgsRef(theta, lr, history, tolerance_grad, tolerance_change, stop_loss, ring_dtype)
        self.c1, self.c2, self.max_ls = float(c1), float(c2), int(max_ls)
        self.f32 = self.lb.ring_dtype == np.float32
        self.theta0 = self.lb.theta.copy()
        self.theta = self.theta0.copy()                  # where the next evaluation is taken
        self.state = IDLE
        self.t = 0.0
        self.b, self.bf, self.bgtd, self.bslot = [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [START_SLOT, START_SLOT]
        self.low_pos, self.insuf = 0, False
        self.ls_iter = self.ls_evals = self.evals_total = 0
        self.f0 = self.gtd0 = self.dnorm = 0.0
        self.slot_new = 0
        self.slot_g = [None, None, None]
        self.accepted = self.end_max_ls = self.end_width = self.end_curv = self.stalled = 0
        self.margins = []
        self.phase = 0
        self.gtd_scale = 0.0                             # the largest sum |g_i d_i| seen: what a dot product's rounding error scales with

    # ---- comparisons with a recorded margin ----------------------------------------------------------------------------------
    def _m(self, a, b, scale=None, exact_ok=False):
        if exact_ok and a == b:
            return
        s = max(abs(a), abs(b)) if scale is None else scale
        self.margins.append(abs(a - b) / s if s > 0 and np.isfinite(a - b) else 0.0)

    def _armijo_scale(self, t):
        # both sides fed the SAME losses: of f0 + c1 t g0.d only the last term can differ between them
        return abs(self.c1 * t * self.gtd0) if self.exact_losses else None

    def _point(self, t):
        p = self.theta0 + t * self.lb.d
        return p.astype(np.float32).astype(np.float64) if self.f32 else p

    def _cubic(self, x1, f1, g1, x2, f2, g2, bounds=None):
        """torch.optim.lbfgs._cubic_interpolate"""
        if bounds is not None:
            lo, hi = bounds
        else:
            lo, hi = (x1, x2) if x1 <= x2 else (x2, x1)
        with np.errstate(all="ignore"):
            return self._cubic_body(x1, f1, g1, x2, f2, g2, lo, hi)

    def _cubic_body(self, x1, f1, g1, x2, f2, g2, lo, hi):
        d1 = g1 + g2 - 3 * (f1 - f2) / (x1 - x2)
        d2_square = d1 ** 2 - g1 * g2
        self._m(d1 ** 2, g1 * g2, scale=d1 ** 2 + abs(g1 * g2))
        if d2_square >= 0:
            d2 = np.sqrt(d2_square)
            if x1 <= x2:
                min_pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2))
            else:
                min_pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2 * d2))
            self._m(min_pos, lo); self._m(min_pos, hi)
            return min(max(min_pos, lo), hi)
        return (lo + hi) / 2.0

    def _free_slot(self, live):
        return next(s for s in (0, 1, 2) if s not in live)

    # ---- one evaluation ---------------------------------------------------------------------------------------------------------
    def tick(self, loss, g):
        """Consume the evaluation (loss, g) at self.theta.  -> the record (see _out)."""
        lb = self.lb
        self.margins = []
        if lb.frozen:
            return self._out(None, wrote=False)
        g = np.asarray(g, np.float64)
        loss = float(loss)
        self.evals_total += 1
        slot = self.slot_new
        self.slot_g[slot] = g.copy()
        if self.state == IDLE:
            return self._accept(0.0, loss, 0.0, slot, idle=True)
        gtd_new = float(g @ lb.d)
        scale = float(np.abs(g * lb.d).sum())
        self.gtd_scale = max(self.gtd_scale, scale)
        if self.ls_evals == 0:
            self.dnorm = float(np.abs(lb.d).max())
        self.ls_evals += 1
        if not (np.isfinite(loss) and np.isfinite(np.abs(g).sum())):
            t_low = self.b[self.low_pos] if self.state == ZOOM else 0.0
            self.theta0 = self._point(t_low)
            self.theta = self.theta0.copy()
            lb.theta = self.theta0.copy()
            lb.frozen = FROZEN_NONFINITE
            self.state = IDLE
            self.phase = 4
            return self._out(None)
        t, f0, gtd0, c1, c2 = self.t, self.f0, self.gtd0, self.c1, self.c2
        b, bf, bgtd, bslot = self.b, self.bf, self.bgtd, self.bslot
        done = False
        if self.state == BRACKET:
            if self.ls_iter < self.max_ls:
                armijo = f0 + c1 * t * gtd0
                self._m(loss, armijo, scale=self._armijo_scale(t))
                to_zoom = loss > armijo
                if not to_zoom and self.ls_iter > 1:
                    self._m(loss, bf[0], exact_ok=True)
                    to_zoom = loss >= bf[0]
                if not to_zoom:
                    self._m(abs(gtd_new), -c2 * gtd0, scale=scale)
                    if abs(gtd_new) <= -c2 * gtd0:
                        self.end_curv += 1
                        return self._accept(t, loss, gtd_new, slot)
                    self._m(gtd_new, 0.0, scale=scale)
                    to_zoom = gtd_new >= 0
                if not to_zoom:
                    t_next = self._cubic(b[0], bf[0], bgtd[0], t, loss, gtd_new, bounds=(t + 0.01 * (t - b[0]), t * 10))
                    b[0], bf[0], bgtd[0], bslot[0] = t, loss, gtd_new, slot
                    self.ls_iter += 1
                    self.t = t_next
                    self.slot_new = self._free_slot((slot,))
                    self.theta = self._point(t_next)
                    self.phase = 1
                    return self._out(None)
                b[1], bf[1], bgtd[1], bslot[1] = t, loss, gtd_new, slot
            else:                                        # torch: "reached max number of iterations": the bracket [0, t]
                b[0], bf[0], bgtd[0], bslot[0] = 0.0, f0, gtd0, START_SLOT
                b[1], bf[1], bgtd[1], bslot[1] = t, loss, gtd_new, slot
            self.insuf = False
            self.low_pos = 0 if bf[0] <= bf[1] else 1
        else:
            self.ls_iter += 1
            low = self.low_pos
            high = 1 - low
            armijo = f0 + c1 * t * gtd0
            self._m(loss, armijo, scale=self._armijo_scale(t))
            up = loss > armijo
            if not up:
                self._m(loss, bf[low], exact_ok=True)
                up = loss >= bf[low]
            if up:
                b[high], bf[high], bgtd[high], bslot[high] = t, loss, gtd_new, slot
                self.low_pos = 0 if bf[0] <= bf[1] else 1
            else:
                self._m(abs(gtd_new), -c2 * gtd0, scale=scale)
                if abs(gtd_new) <= -c2 * gtd0:
                    done = True
                else:
                    self._m(gtd_new, 0.0, scale=scale)
                    if gtd_new * (b[high] - b[low]) >= 0:
                        b[high], bf[high], bgtd[high], bslot[high] = b[low], bf[low], bgtd[low], bslot[low]
                b[low], bf[low], bgtd[low], bslot[low] = t, loss, gtd_new, slot
        # the head of torch's zoom loop
        low = self.low_pos
        if done:
            self.end_curv += 1
            return self._accept(b[low], bf[low], bgtd[low], bslot[low])
        if self.ls_iter >= self.max_ls:
            self.end_max_ls += 1
            return self._accept(b[low], bf[low], bgtd[low], bslot[low])
        width = abs(b[1] - b[0]) * self.dnorm
        self._m(width, lb.tolerance_change)
        if width < lb.tolerance_change:
            self.end_width += 1
            return self._accept(b[low], bf[low], bgtd[low], bslot[low])
        t = self._cubic(b[0], bf[0], bgtd[0], b[1], bf[1], bgtd[1])
        bmax, bmin = max(b), min(b)
        eps = 0.1 * (bmax - bmin)
        self._m(min(bmax - t, t - bmin), eps, exact_ok=True)
        if min(bmax - t, t - bmin) < eps:
            if self.insuf or t >= bmax or t <= bmin:
                t = bmax - eps if abs(t - bmax) < abs(t - bmin) else bmin + eps
                self.insuf = False
            else:
                self.insuf = True
        else:
            self.insuf = False
        self.t = t
        self.state = ZOOM
        self.slot_new = self._free_slot(bslot)
        self.theta = self._point(t)
        self.phase = 2
        return self._out(None)

    def _accept(self, t_acc, f_acc, gtd_acc, slot, idle=False):
        lb = self.lb
        g_acc = lb.g_prev if slot == START_SLOT else self.slot_g[slot]
        if idle:
            self.theta0 = self.theta.copy()
        else:
            self.accepted += 1
            if t_acc == 0.0:
                self.stalled += 1
            self.theta0 = self._point(t_acc)
            lb.t = t_acc
        lb.theta = self.theta0.copy()
        rec = lb.iterate(f_acc, g_acc)
        self.state = IDLE
        self.theta = self.theta0.copy()
        if rec["status"] == "frozen":
            self.phase = 4
            return self._out(rec, t_acc=t_acc)
        self.f0, self.gtd0, self.t = f_acc, rec["gtd"], rec["t"]
        # end 1 keeps, until a bracket forms, the point the search just ended accepted (step, loss, g.d along the old direction)
        self.b, self.bf, self.bgtd, self.bslot = [0.0, t_acc], [f_acc, f_acc], [rec["gtd"], gtd_acc], [START_SLOT, START_SLOT]
        self.low_pos, self.insuf, self.ls_iter, self.ls_evals, self.slot_new = 0, False, 0, 0, 0
        if rec["status"] == "applied":
            self.state = BRACKET
            self.theta = self._point(self.t)
        lb.theta = self.theta.copy()
        self.phase = 3
        return self._out(rec, t_acc=t_acc)

    def _out(self, rec, t_acc=None, wrote=True):
        """phase: what this tick did; t_next: the step of the next trial (the new direction's first step after an accept); iterated:
        whether an L-BFGS iteration ran, `iteration` its record; t_acc: the accepted step; theta: where the next evaluation is taken."""
        return dict(phase=PHASES[self.phase] if wrote else "frozen", t_next=self.t, ls_iter=self.ls_iter, ls_evals=self.ls_evals,
                    evals_total=self.evals_total, t_prev=self.b[0] if self.state == BRACKET else 0.0,
                    b=tuple(self.b), bf=tuple(self.bf), bgtd=tuple(self.bgtd), bslot=tuple(self.bslot), low_pos=self.low_pos,
                    insuf_progress=int(self.insuf), f0=self.f0, gtd0=self.gtd0, dnorm=self.dnorm, slot_new=self.slot_new,
                    accepted=self.accepted, end_max_ls=self.end_max_ls, end_width=self.end_width, end_curv=self.end_curv,
                    stalled=self.stalled, frozen=self.lb.frozen, gtd_scale=self.gtd_scale, iterated=rec is not None and rec["status"] != "frozen", iteration=rec,
                    t_acc=t_acc, margins=list(self.margins), min_margin=min(self.margins) if self.margins else float("inf"),
                    theta=self.theta.copy(), theta0=self.theta0.copy(), wrote=wrote)

    def resync(self, theta0, S, Y, g_prev, d):
        """After an accepted tick: take over the device's fp32 start point, pairs, start gradient and direction; the next trial point
        follows from them."""
        self.lb.load(theta0, S, Y, g_prev, d)
        self.theta0 = np.asarray(theta0, np.float64).copy()
        self.theta = self._point(self.t) if self.state == BRACKET else self.theta0.copy()
        self.lb.theta = self.theta.copy()


def run_flat(ref, fun, n_ticks):
    """n_ticks times "evaluate at ref.theta, tick" on fun(theta) -> (loss, g); -> list of the ticks' records."""
    outs = []
    for _ in range(n_ticks):
        loss, g = fun(ref.theta)
        outs.append(ref.tick(loss, g))
    return outs
