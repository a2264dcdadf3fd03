"""tests/lbfgs_ref.py against torch.optim.LBFGS in float64, no device: the flat loop "evaluate, iterate" IS torch's optimiser without a
line search.  On a smooth non-convex function (parameters to 1e-12, every closure loss to 1e-10) and on scripted (loss, gradient)
sequences fed through a closure that pops the next pair: with max_iter = 1 torch evaluates exactly once per iteration, so the script
lines up with the flat loop whatever branch an iteration takes.  Where the reference's own rules go beyond torch's (the freeze is for
good; a non-finite loss freezes) the script ends at that iteration and the rule itself is asserted."""
import numpy as np
import pytest
import torch

from tests import lbfgs_ref as lr_


def fun(theta):
    """smooth, non-convex: a quartic bowl with a sine ripple"""
    t = torch.as_tensor(theta, dtype=torch.float64).clone().requires_grad_(True)
    k = torch.arange(1, t.numel() + 1, dtype=torch.float64)
    f = (0.25 * (t ** 4).sum() + 0.5 * (k * (t - 0.3) ** 2).sum() / t.numel() + 0.3 * torch.sin(3.0 * t + 0.1 * k).sum())
    f.backward()
    return float(f), t.grad.numpy().copy()


def torch_run(theta0, lr, history, outer, max_iter, tolerance_grad=1e-7, tolerance_change=1e-9):
    th = torch.tensor(theta0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.LBFGS([th], lr=lr, max_iter=max_iter, history_size=history, tolerance_grad=tolerance_grad,
                            tolerance_change=tolerance_change)
    losses = []

    def closure():
        opt.zero_grad()
        l, g = fun(th.detach().numpy())
        th.grad = torch.from_numpy(g)
        losses.append(l)
        return torch.tensor(l, dtype=torch.float64)

    for _ in range(outer):
        opt.step(closure)
    return th.detach().numpy().copy(), losses


@pytest.mark.parametrize("history,outer,max_iter,lr,tol_grad", [(3, 6, 4, 0.05, 1e-7), (100, 3, 20, 0.05, 1e-7), (10, 40, 5, 0.5, 1e-3)],
                         ids=["h3_6x4", "h100_3x20", "converging_40x5"])
def test_flat_loop_is_torch_on_a_smooth_function(history, outer, max_iter, lr, tol_grad):
    theta0 = np.random.default_rng(1).normal(0, 0.7, 24)
    want, losses = torch_run(theta0, lr, history, outer, max_iter, tolerance_grad=tol_grad)
    ref = lr_.LbfgsRef(theta0, lr, history, tolerance_grad=tol_grad)
    flat_losses = []
    # torch re-evaluates at unchanged parameters when an outer call ended early: the flat loop sees every DISTINCT evaluation once
    for _ in range(outer * max_iter):
        l, g = fun(ref.theta)
        flat_losses.append(l)
        ref.iterate(l, g)
    assert np.abs(ref.theta - want).max() <= 1e-12, np.abs(ref.theta - want).max()
    distinct = [l for i, l in enumerate(losses) if i == 0 or l != losses[i - 1]]
    flat_distinct = [l for i, l in enumerate(flat_losses) if i == 0 or l != flat_losses[i - 1]]
    n = min(len(distinct), len(flat_distinct))
    assert n >= min(len(distinct), outer)
    assert np.abs(np.array(distinct[:n]) - np.array(flat_distinct[:n])).max() <= 1e-10
    if tol_grad > 1e-7:
        assert ref.frozen == lr_.FROZEN_GRAD and ref.n_iter < outer * max_iter, (ref.frozen, ref.n_iter)      # converges and stops for good


def scripted(script, theta0, lr, history, tolerance_grad=1e-7, tolerance_change=1e-9):
    """torch (max_iter = 1: one closure evaluation per step) and the flat reference on the same scripted pairs -> per-step thetas of both"""
    th = torch.tensor(theta0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.LBFGS([th], lr=lr, max_iter=1, history_size=history, tolerance_grad=tolerance_grad, tolerance_change=tolerance_change)
    feed = list(script)

    def closure():
        l, g = feed.pop(0)
        th.grad = torch.as_tensor(g, dtype=torch.float64).clone()
        return torch.tensor(l, dtype=torch.float64)

    ref = lr_.LbfgsRef(theta0, lr, history, tolerance_grad, tolerance_change)
    rows = []
    for l, g in script:
        opt.step(closure)
        out = ref.iterate(l, g)
        rows.append((th.detach().numpy().copy(), out))
    assert not feed
    return rows, ref, opt


def quad_script(rng, P, n, scale=1.0):
    """gradients of a convex quadratic along a made-up path: pairs with ys > 0 mostly"""
    A = rng.normal(0, 1, (P, P)); A = A @ A.T / P + np.eye(P)
    return [(float(n - i), scale * A @ rng.normal(0, 1, P)) for i in range(n)]


def test_scripted_ring_wrap_and_rejected_pairs():
    rng = np.random.default_rng(2)
    P = 12
    script = quad_script(rng, P, 14)
    script[5] = (script[5][0], script[4][1].copy())                  # y = 0: ys = 0 fails ys > 1e-10
    script[9] = (script[9][0], script[8][1] * (1 - 1e-9))            # ys tiny / of either sign
    rows, ref, _ = scripted(script, rng.normal(0, 1, P), 0.1, history=3)
    pushed = [o["pushed"] for _, o in rows]
    counts = [o["count"] for _, o in rows]
    assert pushed[5] == 0 and counts[5] == counts[4]                 # the rejected pair left the ring as it was
    assert max(counts) == 3 and sum(pushed) > 3                      # the ring wrapped
    for k, (want, o) in enumerate(rows):
        assert np.abs(o["theta"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (k, o["status"])


def test_scripted_gtd_skip():
    rng = np.random.default_rng(3)
    P = 8
    script = quad_script(rng, P, 8)
    theta0 = rng.normal(0, 1, P)
    # a huge tolerance_change: every direction has g.d > -tolerance_change -> no update, state carried on
    rows, ref, _ = scripted(script, theta0, 0.1, history=4, tolerance_change=1e12)
    for want, o in rows:
        assert o["status"] == "skipped"
        np.testing.assert_array_equal(want, theta0)
        np.testing.assert_array_equal(o["theta"], theta0)
    assert ref.n_iter == len(script)
    # mixed: the skip of one step only (a tiny gradient -> g.d ~ -1e-24 > -1e-9 but max|g| above tolerance_grad)
    script = quad_script(rng, P, 8)
    script[4] = (script[4][0], np.full(P, 1e-12))
    rows, ref, _ = scripted(script, theta0, 0.1, history=4, tolerance_grad=1e-13)
    assert rows[4][1]["status"] == "skipped" and rows[5][1]["status"] in ("applied", "skipped")
    for k, (want, o) in enumerate(rows):
        assert np.abs(o["theta"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (k, o["status"])


def test_scripted_tolerance_grad_freeze_is_for_good():
    rng = np.random.default_rng(4)
    P = 8
    script = quad_script(rng, P, 5)
    script.append((0.5, np.full(P, 1e-8)))                           # max|g| <= 1e-7: torch returns before touching anything
    rows, ref, _ = scripted(script, rng.normal(0, 1, P), 0.1, history=4)
    for want, o in rows:
        assert np.abs(o["theta"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert rows[-1][1]["status"] == "frozen" and ref.frozen == lr_.FROZEN_GRAD
    np.testing.assert_array_equal(rows[-1][1]["theta"], rows[-2][1]["theta"])
    frozen_theta, n_iter = ref.theta.copy(), ref.n_iter
    out = ref.iterate(1.0, rng.normal(0, 1, P))                      # the engine's rule: frozen for good, whatever comes
    assert out["status"] == "frozen" and ref.n_iter == n_iter
    np.testing.assert_array_equal(ref.theta, frozen_theta)


def test_scripted_nan_loss_freezes():
    rng = np.random.default_rng(5)
    P = 8
    script = quad_script(rng, P, 4)
    rows, ref, _ = scripted(script, rng.normal(0, 1, P), 0.1, history=4)
    for want, o in rows:
        assert np.abs(o["theta"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    before = ref.theta.copy()
    for bad_loss, bad_g in ((float("nan"), rng.normal(0, 1, P)), (1.0, np.r_[np.inf, np.zeros(P - 1)])):
        r2 = lr_.LbfgsRef(before, 0.1, 4)
        out = r2.iterate(bad_loss, bad_g)                            # torch has no such check; the engine's rule
        assert out["status"] == "frozen" and r2.frozen == lr_.FROZEN_NONFINITE and r2.n_iter == 0
        np.testing.assert_array_equal(r2.theta, before)


def test_stop_loss_freezes_and_fp32_ring_stays_close():
    rng = np.random.default_rng(6)
    P = 16
    theta0 = rng.normal(0, 0.7, P)
    a = lr_.LbfgsRef(theta0, 0.05, 6)
    b = lr_.LbfgsRef(theta0, 0.05, 6, ring_dtype=np.float32)
    lr_.run_flat(a, fun, 12)
    lr_.run_flat(b, fun, 12)
    assert 0 < np.abs(a.theta - b.theta).max() < 1e-4                # fp32 pairs: the same iteration, rounded storage
    c = lr_.LbfgsRef(theta0, 0.05, 6, stop_loss=1e30)
    out = c.iterate(*fun(theta0))
    assert out["status"] == "frozen" and c.frozen == lr_.FROZEN_LOSS
