"""Float64 reference of ONE optimiser update as the engine's C ABI describes it (include/gpe_hip.h: gpe_config "optimiser" and
"early stopping" comments, gpe_scalars, GPE_ERR_NONFINITE) and as the reference scripts run it per epoch:

    torch.nn.utils.clip_grad_norm_(params, clip_norm)      refine/harmonic_pinn_simulation.py:359
    torch.optim.Adam(lr, betas, eps).step()                :309, :360
    scheduler.step(total_loss)                             :361  (CosineAnnealingWarmRestarts fed the LOSS as the epoch, quirk Q4)
                                                           nb c10:L76-78, L103 (ReduceLROnPlateau, mode 'min', relative threshold)
    early stopping on the loss                             :363-400

A checker, not product code: plain numpy in double precision, no fused steps, every intermediate of the Adam element returned so that a
test can form round-off bounds for an fp32 implementation from them.  tests/test_update_reference_cpu.py holds this file to torch's own
clip_grad_norm_ / Adam / CosineAnnealingWarmRestarts / ReduceLROnPlateau and to gpe_oracle.optimizer_step.
"""
from __future__ import annotations

import math

import numpy as np

SCHED_CONST, SCHED_COSINE_LOSS, SCHED_PLATEAU = 0, 1, 2


def cosine_cycle(epoch: float, T_0: float, T_mult: float):
    """(n, T_cur, T_i) of CosineAnnealingWarmRestarts.step(epoch) for a fractional epoch: the index of the restart cycle the epoch
    falls in, the position inside it and its length.  Cycle n starts at T_0 (T_mult^n - 1) / (T_mult - 1) and lasts T_0 T_mult^n
    (T_mult = 1: starts at n T_0, lasts T_0)."""
    if epoch < T_0:
        return 0, epoch, T_0
    if T_mult == 1:
        return int(epoch // T_0), math.fmod(epoch, T_0), T_0
    n = int(math.log(epoch / T_0 * (T_mult - 1) + 1, T_mult))
    return n, epoch - T_0 * (T_mult ** n - 1) / (T_mult - 1), T_0 * T_mult ** n


class UpdateRef:
    """State machine of the update.  Every configuration number is taken as given (a test that compares with an fp32 engine passes
    the fp32-rounded values); all arithmetic is float64."""

    def __init__(self, theta, *, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clip_norm=1.0, sched=SCHED_CONST, T_0=200.0, T_mult=2.0,
                 eta_min=1e-6, factor=0.5, patience=100, min_lr=1e-5, threshold=1e-4, stop_tol=0.0, stop_patience=0):
        self.beta1, self.beta2, self.eps, self.clip_norm = float(beta1), float(beta2), float(eps), float(clip_norm)
        self.sched, self.T_0, self.T_mult, self.eta_min = int(sched), float(T_0), float(T_mult), float(eta_min)
        self.factor, self.patience, self.min_lr, self.threshold = float(factor), int(patience), float(min_lr), float(threshold)
        self.stop_tol, self.stop_patience = float(stop_tol), int(stop_patience)
        self.theta = np.array(theta, dtype=np.float64).ravel()
        self.history = []                     # one record per APPLIED step, in order
        self.reset_optimizer(lr)

    # ---- state ---------------------------------------------------------------------------------------------------------
    def reset_optimizer(self, lr):
        """New Adam + scheduler + early-stop state (a new optimiser object per continuation stage); the parameters stay."""
        self.lr = self.lr0 = float(lr)
        self.m = np.zeros_like(self.theta)
        self.v = np.zeros_like(self.theta)
        self.step = 0
        self.b1p = self.b2p = 1.0             # beta^step, kept as running products
        self.best, self.num_bad = math.inf, 0                      # plateau scheduler
        self.es_best, self.es_count = math.inf, 0                  # early stop
        self.stopped, self.stop_step = False, 0
        self.nonfinite = False                # sticky
        self.last = None                      # record of the most recent update that was not frozen

    def set_adam_state(self, m, v, step):
        self.m = np.array(m, dtype=np.float64).ravel()
        self.v = np.array(v, dtype=np.float64).ravel()
        self.step = int(step)
        self.b1p, self.b2p = self.beta1 ** self.step, self.beta2 ** self.step

    # ---- schedulers ----------------------------------------------------------------------------------------------------
    def _sched_step(self, loss):
        if self.sched == SCHED_COSINE_LOSS:
            epoch = float(np.float32(loss))   # the reference hands the scheduler its fp32 loss tensor
            _, T_cur, T_i = cosine_cycle(epoch, self.T_0, self.T_mult)
            self.lr = self.eta_min + (self.lr0 - self.eta_min) * (1 + math.cos(math.pi * T_cur / T_i)) / 2
        elif self.sched == SCHED_PLATEAU:
            if loss < self.best * (1 - self.threshold):
                self.best, self.num_bad = loss, 0
            else:
                self.num_bad += 1
            if self.num_bad > self.patience:
                new_lr = max(self.lr * self.factor, self.min_lr)
                if self.lr - new_lr > 1e-8:
                    self.lr = new_lr
                self.num_bad = 0

    # ---- one update ----------------------------------------------------------------------------------------------------
    def update(self, grad, loss, mse_mode=False):
        """grad: the gradient before clipping; loss: the value the step recorded.  Returns the intermediates of the step:
        status ('applied' | 'skipped' | 'frozen'), grad_norm, coef, lr (the one this step used), ss = lr / (1 - beta1^t),
        g (clipped gradient), m, v (new moments), denom, upd = ss m / denom, theta (new parameters)."""
        g_raw = np.asarray(grad, dtype=np.float64).ravel()
        loss = float(loss)
        gn = math.sqrt(float(np.sum(g_raw * g_raw)))
        if self.stopped:                      # after the stopping step nothing moves and nothing is recorded
            return dict(status="frozen", grad_norm=gn)
        if not (math.isfinite(loss) and math.isfinite(gn)):
            self.nonfinite = True
            self.last = dict(step=self.step, loss=loss, grad_norm=gn, lr=self.lr, nonfinite=True)
            return dict(status="skipped", grad_norm=gn)
        coef = 1.0
        if self.clip_norm > 0 and not mse_mode:
            coef = min(1.0, self.clip_norm / (gn + 1e-6))
        g = g_raw * coef
        self.step += 1
        self.b1p *= self.beta1
        self.b2p *= self.beta2
        self.m = self.m + (g - self.m) * (1 - self.beta1)
        self.v = self.v * self.beta2 + (1 - self.beta2) * g * g
        lr = self.lr
        ss = lr / (1 - self.b1p)
        denom = np.sqrt(self.v) / math.sqrt(1 - self.b2p) + self.eps
        upd = ss * (self.m / denom)
        self.theta = self.theta - upd
        rec = dict(step=self.step, loss=loss, grad_norm=gn, lr=lr, nonfinite=False)
        self.last = rec
        self.history.append(rec)
        if not mse_mode:
            if loss < self.es_best:
                self.es_best, self.es_count = loss, 0
            else:
                self.es_count += 1
            if (self.stop_tol > 0 and loss <= self.stop_tol) or (self.stop_patience > 0 and self.es_count >= self.stop_patience):
                self.stopped, self.stop_step = True, self.step
            self._sched_step(loss)
        return dict(status="applied", grad_norm=gn, coef=coef, lr=lr, ss=ss, g=g, m=self.m, v=self.v, denom=denom, upd=upd,
                    theta=self.theta)
