"""tests/lbfgs_ls_ref.py against torch.optim.LBFGS(line_search_fn="strong_wolfe") in float64, no device.  One opt.step(closure) with
max_iter = K and max_eval = 10**6 logs (theta, loss, n_iter) per closure call; the flat machine is fed the same objective, one tick per
logged call: the same number of evaluations per iteration, every trial theta and the final theta to 1e-12 relative.  torch hands
`_strong_wolfe` its default tolerance_change = 1e-9 whatever the optimiser's is, so both sides run with 1e-9 here.

The ends of a search are driven on 1-D profiles through torch's `_strong_wolfe` itself and through the flat machine, and which end was
taken is asserted, so a profile that stops reaching its branch fails.

Last, the seeds of the GPU test's tick-by-tick cells (tests/lbfgs_ls_cases.py): the reference ALONE, in the device's fp32 storage and fed
what the device is fed, keeps every decision margin above 1e-6 on every tick."""
import numpy as np
import pytest
import torch
from torch.optim.lbfgs import _strong_wolfe

from tests import lbfgs_ls_cases as cases
from tests import lbfgs_ls_ref as ls_


def quadratic(P, seed):
    rng = np.random.default_rng(seed)
    a, star = rng.uniform(0.5, 2.0, P), rng.normal(0, 1, P)
    return (lambda th: (0.5 * float(np.sum(a * (th - star) ** 2)), a * (th - star))), rng.normal(0, 1, P)


def rosenbrock(P, seed):
    theta0 = np.random.default_rng(seed).uniform(-1.2, 1.2, P)
    obj = cases.Rosenbrock(np.zeros(P), seed)
    obj.shift = np.zeros(P)
    return obj, theta0


def mlp(P, seed):
    """1-6-3-1 tanh network (6 + 6 + 18 + 3 + 3 + 1 = 37 weights and biases, padded by three quadratic parameters to 40) fitted to sin"""
    assert P == 40
    x = torch.linspace(-2, 2, 32, dtype=torch.float64).reshape(-1, 1)
    y = torch.sin(2 * x)

    def fun(th):
        t = torch.as_tensor(th, dtype=torch.float64).clone().requires_grad_(True)
        W1, b1, W2, b2, W3, b3, rest = t[0:6].reshape(1, 6), t[6:12], t[12:30].reshape(6, 3), t[30:33], t[33:36].reshape(3, 1), t[36:37], t[37:]
        out = torch.tanh(torch.tanh(x @ W1 + b1) @ W2 + b2) @ W3 + b3
        f = ((out - y) ** 2).mean() + 0.5 * (rest ** 2).sum()
        f.backward()
        return float(f.detach()), t.grad.numpy().copy()

    return fun, np.random.default_rng(seed).normal(0, 0.7, P)


PROBLEMS = {"quadratic": (quadratic, 24), "rosenbrock": (rosenbrock, 16), "mlp": (mlp, 40)}


def torch_log(fun, theta0, lr, history, K):
    th = torch.tensor(theta0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.LBFGS([th], lr=lr, max_iter=K, max_eval=10 ** 6, history_size=history, tolerance_grad=1e-7, tolerance_change=1e-9,
                            line_search_fn="strong_wolfe")
    log = []

    def closure():
        l, g = fun(th.detach().numpy().copy())
        th.grad = torch.from_numpy(g.copy())
        log.append((th.detach().numpy().copy(), l, opt.state[opt._params[0]].get("n_iter", 0)))
        return torch.tensor(l, dtype=torch.float64)

    opt.step(closure)
    return th.detach().numpy().copy(), log


@pytest.mark.parametrize("history", [3, 10])
@pytest.mark.parametrize("lr", [0.01, 1.0, 8.0])
@pytest.mark.parametrize("problem", list(PROBLEMS))
def test_flat_machine_is_torch_with_strong_wolfe(problem, lr, history):
    make, P = PROBLEMS[problem]
    fun, theta0 = make(P, 7)
    K = 12
    final, log = torch_log(fun, theta0, lr, history, K)
    ref = ls_.LbfgsLsRef(theta0, lr, history, tolerance_grad=1e-7, tolerance_change=1e-9, max_ls=25)
    per_iter_ref, phases = {}, set()
    for k, (theta, loss, n_iter) in enumerate(log):
        scale = max(1.0, np.abs(theta).max())
        assert np.abs(ref.theta - theta).max() <= 1e-12 * scale, (k, np.abs(ref.theta - theta).max())
        l, g = fun(ref.theta)
        # the iteration this evaluation belongs to, as torch counts it (the very first call comes before iteration 1)
        it = ref.lb.n_iter if k else 0
        per_iter_ref[it] = per_iter_ref.get(it, 0) + 1
        out = ref.tick(l, g)
        phases.add(out["phase"])
    per_iter_torch = {}
    for _, _, n_iter in log:
        per_iter_torch[n_iter] = per_iter_torch.get(n_iter, 0) + 1
    assert per_iter_ref == per_iter_torch, (per_iter_ref, per_iter_torch)
    assert out["phase"] in ("accepted", "frozen")                    # torch's last evaluation ends a search
    assert np.abs(ref.theta0 - final).max() <= 1e-12 * max(1.0, np.abs(final).max())
    assert len(log) >= 4 and max(per_iter_torch) >= 2, per_iter_torch
    print(f"[{problem} lr={lr} m={history}] evaluations per iteration {[per_iter_torch[k] for k in sorted(per_iter_torch)]} phases {sorted(phases)}")
    if problem == "quadratic" and lr == 0.01:
        assert "bracket" in phases and per_iter_torch[1] >= 3         # the bracket phase extrapolates
    if problem == "quadratic" and lr == 8.0:
        assert "zoom" in phases                                       # Armijo fails, zoom


# ---- the ends of a search on 1-D profiles ------------------------------------------------------------------------------------------
def both_on_profile(phi, dphi, t, max_ls, tolerance_change=1e-9):
    """torch's _strong_wolfe and the flat machine on f(x) = phi(x) from x = 0 along d = 1 with first step t.
    -> (torch's (f, g, t, evals), the flat machine's accepting record, the steps it evaluated)"""
    x0 = torch.zeros(1, dtype=torch.float64)
    d = torch.ones(1, dtype=torch.float64)

    def obj(x, tt, dd):
        p = float(x[0] + tt * dd[0])
        return phi(p), torch.tensor([dphi(p)], dtype=torch.float64)

    f0, g0 = phi(0.0), dphi(0.0)
    want = _strong_wolfe(obj, x0, t, d, f0, torch.tensor([g0], dtype=torch.float64), g0, tolerance_change=tolerance_change, max_ls=max_ls)
    ref = ls_.LbfgsLsRef(np.zeros(1), 1.0, 3, tolerance_grad=0.0, tolerance_change=tolerance_change, max_ls=max_ls)
    # put the machine at the start of this search: direction 1, first step t (the first tick of a run would choose both itself)
    ref.lb.n_iter, ref.lb.d, ref.lb.g_prev, ref.lb.t = 1, np.ones(1), np.array([g0]), t
    ref.f0, ref.gtd0, ref.t, ref.bf, ref.bgtd, ref.state = f0, g0, t, [f0, 0.0], [g0, 0.0], ls_.BRACKET
    ref.theta = ref._point(t)
    steps = []
    for _ in range(200):
        steps.append(float(ref.theta[0]))
        out = ref.tick(phi(steps[-1]), np.array([dphi(steps[-1])]))
        if out["phase"] in ("accepted", "frozen"):
            break
    assert len(steps) == want[3], (steps, want[3])
    assert out["t_acc"] == pytest.approx(float(want[2]), rel=1e-12, abs=1e-300) and float(want[0]) == phi(out["t_acc"])
    return want, out, steps


def test_end_max_ls_fallback():
    # a steadily falling line: the bracket phase extrapolates until max_ls = 3, then torch's fallback bracket [0, t]
    want, out, steps = both_on_profile(lambda p: -p, lambda p: -1.0, 0.1, max_ls=3)
    assert out["end_max_ls"] == 1 and out["end_curv"] == 0 and out["end_width"] == 0 and len(steps) == 4
    assert out["t_acc"] == steps[-1] and out["b"][0] == 0.0


def test_end_bracket_width_break():
    # a kink at 0.3: the slope never satisfies the curvature test, the bracket shrinks onto the kink until its width * max|d| < tolerance
    phi, dphi = (lambda p: abs(p - 0.3)), (lambda p: -1.0 if p < 0.3 else 1.0)
    want, out, steps = both_on_profile(phi, dphi, 1.0, max_ls=200, tolerance_change=1e-3)
    assert out["end_width"] == 1 and out["end_curv"] == 0 and out["end_max_ls"] == 0
    assert abs(out["t_acc"] - 0.3) < 1e-3                              # the bracket closed on the kink


def test_insufficient_progress_branch_and_an_accepted_point_that_is_not_the_last():
    # the same kink with a tight budget: the interpolant keeps landing at an end of the bracket (the eps rule moves it 10 % in), and the
    # search ends by max_ls on the lower end, which is not the point evaluated last
    phi, dphi = (lambda p: abs(p - 0.3)), (lambda p: -1.0 if p < 0.3 else 1.0)
    seen = set()
    for max_ls in range(2, 12):
        want, out, steps = both_on_profile(phi, dphi, 1.0, max_ls=max_ls, tolerance_change=1e-12)
        if out["t_acc"] != steps[-1]:
            seen.add("not_last")
            assert out["end_max_ls"] == 1
    assert "not_last" in seen
    # insuf_progress: a flat machine's record shows the flag raised on a tick of a cubic whose minimiser sits just inside an end
    phi, dphi = (lambda p: (p - 0.95) ** 2 + 5.0 * max(0.0, p - 1.0)), (lambda p: 2 * (p - 0.95) + (5.0 if p > 1.0 else 0.0))
    x0 = np.zeros(1)
    ref = ls_.LbfgsLsRef(x0, 1.0, 3, tolerance_grad=0.0, tolerance_change=1e-12, c2=1e-3, max_ls=30)
    ref.lb.n_iter, ref.lb.d, ref.lb.g_prev, ref.lb.t = 1, np.ones(1), np.array([dphi(0.0)]), 1.05
    ref.f0, ref.gtd0, ref.t, ref.bf, ref.bgtd, ref.state = phi(0.0), dphi(0.0), 1.05, [phi(0.0), 0.0], [dphi(0.0), 0.0], ls_.BRACKET
    ref.theta = ref._point(1.05)
    flags, steps = [], []
    for _ in range(30):
        steps.append(float(ref.theta[0]))
        out = ref.tick(phi(steps[-1]), np.array([dphi(steps[-1])]))
        flags.append(out["insuf_progress"])
        if out["phase"] in ("accepted", "frozen"):
            break
    d = torch.ones(1, dtype=torch.float64)
    torch_steps = []

    def obj(x, tt, dd):
        torch_steps.append(float(tt))
        return phi(float(tt)), torch.tensor([dphi(float(tt))], dtype=torch.float64)

    want = _strong_wolfe(obj, torch.zeros(1, dtype=torch.float64), 1.05, d, phi(0.0), torch.tensor([dphi(0.0)], dtype=torch.float64), dphi(0.0),
                         c2=1e-3, tolerance_change=1e-12, max_ls=30)
    assert 1 in flags, (flags, steps)
    np.testing.assert_allclose(steps, torch_steps, rtol=1e-12)
    assert out["t_acc"] == pytest.approx(float(want[2]), rel=1e-12)


def test_nonfinite_trial_restores_the_best_point_and_stall_counts():
    fun, theta0 = quadratic(8, 3)
    ref = ls_.LbfgsLsRef(theta0, 8.0, 3)
    outs = ls_.run_flat(ref, fun, 3)
    assert outs[-1]["phase"] == "zoom"
    t_low = ref.b[ref.low_pos]
    want = ref.theta0 + t_low * ref.lb.d
    out = ref.tick(float("nan"), fun(ref.theta)[1])
    assert out["phase"] == "frozen" and out["frozen"] == 2
    np.testing.assert_array_equal(ref.theta, want)
    again = ref.tick(1.0, fun(ref.theta)[1])
    assert again["phase"] == "frozen" and not again["wrote"]
    np.testing.assert_array_equal(ref.theta, want)
    # a loss that rises wherever it is tried: the bracket closes on t = 0, which is accepted: stalled, theta unchanged, no pair pushed
    ref = ls_.LbfgsLsRef(theta0, 1.0, 3, max_ls=4)
    l0, g0 = fun(theta0)
    ref.tick(l0, g0)
    for k in range(8):
        out = ref.tick(l0 + 1.0 + k, g0)
        if out["phase"] == "accepted":
            break
    assert out["stalled"] == 1 and out["t_acc"] == 0.0 and out["iteration"]["pushed"] == 0
    np.testing.assert_array_equal(ref.theta0, theta0)


@pytest.mark.parametrize("history", [3, 10])
@pytest.mark.parametrize("case", list(cases.TICK_CASES))
@pytest.mark.parametrize("shape", list(cases.SHAPE_PARAMS))
def test_gpu_cells_keep_their_margins_on_the_reference_alone(shape, case, history):
    make, lr, seed = cases.TICK_CASES[case]
    theta0 = cases.start_params(cases.SHAPE_PARAMS[shape])
    obj = make(theta0, seed)
    ref = ls_.LbfgsLsRef(theta0, lr, history, tolerance_grad=1e-30, tolerance_change=1e-9, ring_dtype=np.float32, exact_losses=True)
    outs = ls_.run_flat(ref, lambda th: cases.injected(obj, th), cases.TICKS)
    worst = min(o["min_margin"] for o in outs)
    phases = [o["phase"] for o in outs]
    print(f"[{shape} {case} m={history}] smallest margin {worst:.3e}; {phases}")
    assert cases.TICKS >= 12 and worst > cases.MARGIN_CAP, (worst, phases)
    assert "frozen" not in phases and phases.count("accepted") >= 2
    if case == "quad_lr0.01":
        assert "bracket" in phases
    if case == "quad_lr8":
        assert "zoom" in phases


@pytest.mark.parametrize("name", list(cases.END_CELLS))
def test_gpu_end_cells_reach_their_end_on_the_reference_alone(name):
    phi, dphi, lr, kw, end = cases.END_CELLS[name]
    kw = dict(kw)
    theta0 = cases.start_params(cases.SHAPE_PARAMS["P1153"])
    obj = cases.LineProfile(theta0, phi, dphi)
    ref = ls_.LbfgsLsRef(theta0, lr, 3, tolerance_grad=1e-30, tolerance_change=kw.pop("tolerance_change", 1e-9), ring_dtype=np.float32,
                         exact_losses=True, **kw)
    ref.tick(*cases.injected(obj, ref.theta))
    steps = []
    for _ in range(70):
        steps.append(ref.t)
        out = ref.tick(*cases.injected(obj, ref.theta))
        if out["phase"] in ("accepted", "frozen"):
            break
    assert out["phase"] == "accepted" and out[end] == 1 and out["accepted"] == 1, out
    if name == "not_last":
        assert out["t_acc"] in steps[:-1] and out["t_acc"] != steps[-1]
    if name == "max_ls":
        assert len(steps) == 4 and out["t_acc"] == steps[-1]
