"""The device-resident L-BFGS (csrc/gpe_lbfgs.h: k_lbfgs_dots, k_lbfgs_coef, k_lbfgs_apply behind the update kernel's record launch)
against the flat float64 reference tests/lbfgs_ref.py, which tests/test_lbfgs_reference_cpu.py holds to torch.optim.LBFGS.

Injection (as tests/test_gpu_update_kernel.py): between step_backward() and lbfgs_update() the iteration reads its gradient from
Engine.exchange_grad ([P + 4] fp32) and, with w_pde = 1 and every other weight 0 on N = 256 points, its loss is tail / 256 exactly.

Bound of a single iteration.  The reference is handed the engine's own fp32 state (theta, and the pairs, previous gradient and direction
read back by lbfgs_history) and keeps the rings as the device does (pair rounded to fp32 before its products are taken), so both sides
combine the SAME vectors b_j in {S_j, Y_j, g}: d = sum_j c_j b_j.  With u = 2^-24:
    device   d_f = fl32(sum_j c_j b_j) from an fp64 sum (one rounding: u |d|; the fp64 sum itself is below u^2-level),
             theta' = fl32(theta + t d_f) formed in fp64 (one rounding: u |theta'|)
    =>       |err| <= u |theta'| + u t |d|, doubled as in the update kernel's test:  2 (u |theta'| + u t |d|)
    plus     the coefficients c_j: both sides form them in fp64 from dot products over P terms (error <= P 2^-53 relative to
             sum |a_i b_i| each, and every product here is of vectors without cancellation to speak of: curvatures in [0.5, 2]) and a
             recursion of 2 m dependent stages; tests/lbfgs_ref.direction_from_gram (the device's algebra in numpy) differs from the
             vector two-loop form by < 400 * 2^-53 relative to sum_j |c_j b_j| at P = 33 537, m = 100 on the CPU.  Allowed:
             eps_c = 4 (P + 2 m) 2^-53 (1.5e-11 there), times t sum_j |c_j b_j|.
No tolerance of the single-iteration tests was measured on the GPU.  t, n_iter, the pair count and the flags match exactly; |g|_1 and
max|g| to 1e-10 relative (max|g| is exact).

Whole runs: the loss trajectory of the first 10 iterations against the fp64 reference driven by the fp64 oracle from the same start; the
tolerance is the measured deviation times 4 (profiles/lbfgs/trajectory.txt), written beside each assertion."""
import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import GPEConfig, Engine, GPEError, capi
from oracle import gpe_oracle as go
from tests import lbfgs_ref as lr_
from tests import mse_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N = 256
SHAPES = {
    "P1153": ([1, 32, 32, 1], gpe_pinn.PATH_AUTO),
    "P12737": ([2, 64, 64, 64, 64, 1], gpe_pinn.PATH_AUTO),
    "P33537": ([2, 128, 128, 128, 1], gpe_pinn.PATH_AUTO),
    "generic_P1153": ([1, 32, 32, 1], gpe_pinn.PATH_GENERIC),
}


def make_engine(layers, path=gpe_pinn.PATH_AUTO, seed=5, **kw):
    eng = Engine(GPEConfig(layers=layers, w_pde=1.0, w_bc=0.0, w_norm=0.0, w_sym=0.0, w_orth=0.0, w_riesz=0.0, dx=1.0, path=path, **kw))
    rng = np.random.default_rng(seed)
    eng.bind_points(torch.as_tensor(rng.uniform(-3, 3, (N, layers[0])).astype(np.float32), device="cuda"))
    eng.set_params(rng.normal(0, 0.3, eng.n_params).astype(np.float32))
    return eng


def inject(eng, g, loss=1.0):
    """One L-BFGS iteration that sees the gradient g and the loss float32(256 loss) / 256; returns that loss."""
    P = eng.n_params
    buf = np.zeros(P + 4, np.float32)
    buf[:P] = g
    buf[P] = np.float32(loss * N)
    eng.step_begin()
    eng.step_backward()
    eng.synchronize()
    eng.exchange_grad.copy_(torch.as_tensor(buf, device="cuda"))
    torch.cuda.synchronize()
    eng.lbfgs_update()
    eng.synchronize()
    return float(buf[P]) / N


class Quadratic:
    """g = a (theta - star): curvatures in [0.5, 2] (every pair has ys > 0), gradient entries spanning 1e-12 .. 1e3"""
    def __init__(self, theta0, seed):
        rng = np.random.default_rng(seed)
        P = theta0.size
        self.a = rng.uniform(0.5, 2.0, P)
        self.star = theta0.astype(np.float64) + rng.choice([-1.0, 1.0], P) * 10.0 ** rng.uniform(-12, 3, P)

    def grad(self, theta):
        return (self.a * (theta.astype(np.float64) - self.star)).astype(np.float32)


def synced_iteration(eng, cfg, g, loss, what):
    """Reference loaded with the engine's state, one injected iteration on both, compared within the module docstring's bounds."""
    th0 = eng.get_params()
    S, Y, gp, d = eng.lbfgs_history()
    st0 = eng.lbfgs_read()
    ref = lr_.LbfgsRef(th0, ring_dtype=np.float32, **cfg)
    ref.load(th0, S, Y, gp, d)
    ref.n_iter, ref.t, ref.H_diag, ref.frozen = st0["n_iter"], st0["t"], st0["H_diag"], st0["frozen"]
    loss_in = inject(eng, g, loss)
    r = ref.iterate(loss_in, np.asarray(g, np.float32))
    rec = eng.lbfgs_read()
    th1 = eng.get_params()
    assert rec["n_iter"] == r["n_iter"] and rec["count"] == r["count"] and rec["frozen"] == r["frozen"], (what, rec, r["n_iter"], r["count"])
    assert rec["loss"] == loss_in, (what, rec["loss"], loss_in)
    g64 = np.asarray(g, np.float32).astype(np.float64)
    if np.isfinite(g64).all():
        assert rec["grad_max"] == r["grad_max"], (what, rec["grad_max"], r["grad_max"])
        assert abs(rec["grad_l1"] - r["grad_l1"]) <= 1e-10 * r["grad_l1"], (what, rec["grad_l1"], r["grad_l1"])
    if r["status"] == "frozen":
        np.testing.assert_array_equal(th1, th0, err_msg=what)
        return rec, r
    assert rec["t"] == r["t"] and rec["pushed"] == r["pushed"] and rec["skipped"] == (r["status"] == "skipped"), (what, rec, r["t"], r["status"])
    assert abs(rec["gtd"] - r["gtd"]) <= 1e-9 * abs(r["gtd"]), (what, rec["gtd"], r["gtd"])
    if r["status"] == "skipped":
        np.testing.assert_array_equal(th1, th0, err_msg=what)
        return rec, r
    P, m = th0.size, cfg["history"]
    eps_c = 4.0 * (P + 2 * m) * 2.0 ** -53
    bound = 2 * (U * np.abs(r["theta"]) + U * r["t"] * np.abs(r["d"])) + eps_c * r["t"] * r["absum"]
    err = np.abs(th1.astype(np.float64) - r["theta"])
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    i = int(np.argmax(ratio))
    print(f"[{what}] theta: worst err/bound {ratio[i]:.3f} at element {i} (err {err[i]:.3e}, bound {bound[i]:.3e}); count {r['count']}")
    assert (err <= bound).all(), (what, i, float(err[i]), float(bound[i]))
    assert (th1 != th0).any(), what
    return rec, r


@pytest.mark.parametrize("history", [3, 100])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_single_iterations_against_the_reference(shape, history):
    """Ring counts 0, 1, history - 1, history and the wrap behind it, every one a checked iteration."""
    layers, path = SHAPES[shape]
    eng = make_engine(layers, path)
    cfg = dict(lr=0.1, history=history, tolerance_grad=1e-30, tolerance_change=1e-9)
    eng.lbfgs_config(**cfg)
    q = Quadratic(eng.get_params(), 11)
    checked = {1, 2, 3, history, history + 1, history + 2, history + 3}          # iteration k starts with min(k - 2, history) pairs held
    counts = set()
    for k in range(1, history + 4):
        g = q.grad(eng.get_params())
        if k in checked:
            rec, r = synced_iteration(eng, cfg, g, 1.0 + 1.0 / k, f"{shape} m={history} it={k}")
            assert r["status"] == "applied" and (k == 1 or r["pushed"] == 1), (k, r["status"], r["ys"])
            counts.add(rec["count"])
        else:
            inject(eng, g, 1.0 + 1.0 / k)
    assert {0, 1, history - 1, history} <= counts, counts
    assert eng.lbfgs_read()["count"] == history
    eng.close()


def test_rule_cells():
    layers, path = SHAPES["P1153"]
    eng = make_engine(layers, path)
    cfg = dict(lr=0.1, history=3, tolerance_grad=1e-7, tolerance_change=1e-9)
    eng.lbfgs_config(**cfg)
    q = Quadratic(eng.get_params(), 12)
    for k in range(3):
        g = q.grad(eng.get_params())
        synced_iteration(eng, cfg, g, 2.0, f"rules warm {k}")
    # a rejected pair (y = 0: the same gradient again) leaves the rings as they were
    S0, Y0, _, _ = eng.lbfgs_history()
    rec, r = synced_iteration(eng, cfg, g, 2.0, "rejected pair")
    S1, Y1, _, _ = eng.lbfgs_history()
    assert rec["pushed"] == 0 and r["pushed"] == 0 and rec["ys"] <= 1e-10
    np.testing.assert_array_equal(S0, S1); np.testing.assert_array_equal(Y0, Y1)
    # a gtd skip (g.d ~ -1e-21 > -1e-9, max|g| above tolerance_grad) leaves theta byte-identical, and the iteration counts
    n0 = eng.lbfgs_read()["n_iter"]
    rec, r = synced_iteration(eng, cfg, np.full(eng.n_params, 1e-6, np.float32) * np.sign(g), 2.0, "gtd skip")
    assert r["status"] == "skipped" and rec["skipped"] == 1 and rec["n_iter"] == n0 + 1
    # the freeze (max|g| <= tolerance_grad) persists whatever comes
    rec, r = synced_iteration(eng, cfg, np.full(eng.n_params, 5e-8, np.float32), 2.0, "freeze")
    assert r["status"] == "frozen" and rec["frozen"] == lr_.FROZEN_GRAD
    frozen = eng.get_params()
    hist = eng.lbfgs_history()
    inject(eng, q.grad(frozen), 1.0)
    assert eng.lbfgs_read()["frozen"] == lr_.FROZEN_GRAD and eng.lbfgs_read()["n_iter"] == rec["n_iter"]
    np.testing.assert_array_equal(eng.get_params(), frozen)
    for a, b in zip(hist, eng.lbfgs_history()):
        np.testing.assert_array_equal(a, b)
    # reset_optimizer / set_params clear the state (Adam's too, by its own rule; L-BFGS never touched it)
    m, v, step = eng.get_adam_state()
    assert step == 0 and not m.any() and not v.any()
    eng.reset_optimizer(1e-3)
    st = eng.lbfgs_read()
    assert st["frozen"] == 0 and st["n_iter"] == 0 and st["count"] == 0
    synced_iteration(eng, cfg, q.grad(frozen), 2.0, "after reset")
    assert eng.lbfgs_read()["n_iter"] == 1
    eng.set_params(frozen)
    assert eng.lbfgs_read()["n_iter"] == 0 and eng.lbfgs_history()[0].shape[0] == 0
    # a non-finite gradient, and a non-finite loss, freeze and leave theta untouched
    for bad_g, bad_loss, what in ((np.r_[np.float32("nan"), q.grad(frozen)[1:]], 2.0, "nan gradient"), (q.grad(frozen), float("inf"), "inf loss")):
        eng.lbfgs_config(**cfg)
        synced_iteration(eng, cfg, q.grad(frozen), 2.0, what + " warm")
        th = eng.get_params()
        inject(eng, bad_g, bad_loss)
        assert eng.lbfgs_read()["frozen"] == lr_.FROZEN_NONFINITE, what
        np.testing.assert_array_equal(eng.get_params(), th)
    # stop_loss
    eng.lbfgs_config(stop_loss=0.5, **cfg)
    inject(eng, q.grad(frozen), 0.25)
    assert eng.lbfgs_read()["frozen"] == lr_.FROZEN_LOSS
    np.testing.assert_array_equal(eng.get_params(), th)
    eng.close()


@pytest.mark.parametrize("shape", ["P1153", "P33537"])
def test_forward_after_an_iteration_sees_the_new_weights(shape):
    """The packed weight copies follow the L-BFGS update as they follow the multi-workgroup Adam update (the next k_begin repacks)."""
    layers, path = SHAPES[shape]
    eng = make_engine(layers, path)
    eng.lbfgs_config(lr=0.1, history=3)
    before = eng.get_params()
    inject(eng, np.random.default_rng(7).normal(0, 1, eng.n_params).astype(np.float32), 1.0)
    after = eng.get_params()
    assert (after != before).any()
    x = torch.as_tensor(np.random.default_rng(8).uniform(-3, 3, (64, layers[0])).astype(np.float32), device="cuda")
    got = eng.forward(x).cpu().numpy()
    fresh = Engine(GPEConfig(layers=layers, w_pde=1.0, w_bc=0.0, w_norm=0.0, dx=1.0, path=path))
    fresh.set_params(after)
    np.testing.assert_array_equal(got, fresh.forward(x).cpu().numpy())
    r0 = eng.residual(want_fields=False)
    fresh.bind_points(torch.as_tensor(np.random.default_rng(5).uniform(-3, 3, (N, layers[0])).astype(np.float32), device="cuda"))
    r1 = fresh.residual(want_fields=False)
    r0, r1 = (r[0] if isinstance(r, tuple) else r for r in (r0, r1))
    assert r0["loss"] == r1["loss"]
    eng.close(); fresh.close()


def test_bit_repeatability():
    thetas = []
    for _ in range(2):
        layers, path = SHAPES["P12737"]
        eng = make_engine(layers, path)
        eng.lbfgs_config(lr=0.1, history=4, tolerance_grad=1e-30)
        q = Quadratic(eng.get_params(), 13)
        rng = np.random.default_rng(14)
        for k in range(9):
            inject(eng, q.grad(eng.get_params()) if k % 3 else rng.normal(0, 1, eng.n_params).astype(np.float32), 1.0)
        thetas.append(eng.get_params())
        eng.close()
    np.testing.assert_array_equal(thetas[0], thetas[1])


def _adam_loss_after(eng_factory, n):
    eng = eng_factory()
    for _ in range(n):
        sc = eng.mse_step()
    loss = eng.mse_loss_grad()[0]
    eng.close()
    return loss


def test_whole_run_mse():
    layers = [1, 32, 32, 1]
    x = np.linspace(-4, 4, N).reshape(-1, 1)
    target = (np.pi ** -0.25 * np.exp(-0.5 * x ** 2))                       # phi_0
    flat = np.random.default_rng(21).normal(0, 0.4, go.param_count(layers)).astype(np.float32)
    # L-BFGS step size 0.5: at the driver's lr * 0.1 = 1e-4 an iteration without a line search barely moves the loss (fp64 reference:
    # 7.52 -> 1.23 in 40 iterations; 40 steps of plain Adam -- what mse_step is: no clipping -- at the driver's 1e-3 reach 1.248e-1 in
    # fp64 by oracle.gpe_oracle.optimizer_step(clip_norm=0) and 1.248e-1 on the device); at 0.5 the reference reaches 2.6e-5: a margin of 4800
    lr = 0.5

    def factory():
        e = Engine(GPEConfig(layers=layers, w_bc=0.0, lr=1e-3, sched=capi.SCHED_CONST))
        e.set_params(flat)
        e.bind_points(torch.as_tensor(x.astype(np.float32), device="cuda"))
        e.bind_target(torch.as_tensor(target.astype(np.float32), device="cuda"))
        return e

    eng = factory()
    pb = go.Problem(layers=layers, w_bc=0.0)
    ref = lr_.LbfgsRef(flat, lr, 100)
    want = [o["loss"] for o in lr_.run_flat(ref, lambda th: mse_ref.mse_loss_and_grad(pb, th, x, target), 10)]
    eng.lbfgs_config(lr, history=100)
    got = []
    for _ in range(10):
        eng.lbfgs_run(1, mse=True)
        got.append(eng.lbfgs_read()["loss"])
    eng.lbfgs_run(30, mse=True)
    end = eng.mse_loss_grad()[0]
    rel = max(abs(a - b) / abs(b) for a, b in zip(got, want))
    print(f"[whole run mse] worst relative loss deviation over 10 iterations {rel:.3e}; loss after 40 iterations {end:.6e}")
    assert rel <= MSE_TRAJ_TOL, (rel, got, want)
    adam = _adam_loss_after(factory, 40)
    print(f"[whole run mse] Adam after 40 steps {adam:.6e}")
    assert end < adam, (end, adam)
    eng.close()


def test_whole_run_physics():
    layers = [1, 32, 32, 1]
    x = np.linspace(-4, 4, N).reshape(-1, 1)
    kw = dict(layers=layers, gamma=1.0, p=3, dx=8.0 / N, w_bc=0.0)
    flat = np.random.default_rng(22).normal(0, 0.4, go.param_count(layers)).astype(np.float32)
    eng = Engine(GPEConfig(**kw))
    eng.set_params(flat)
    eng.bind_points(torch.as_tensor(x.astype(np.float32), device="cuda"))
    pb = go.Problem(**kw)

    def fun(th):
        sc, g, _ = go.full_loss_and_grad(pb, th, x)
        return sc["loss"], g

    lr = 1e-2
    ref = lr_.LbfgsRef(flat, lr, 100)
    want = [o["loss"] for o in lr_.run_flat(ref, fun, 10)]
    eng.lbfgs_config(lr, history=100)
    got = []
    for _ in range(10):
        eng.lbfgs_run(1, mse=False)
        got.append(eng.lbfgs_read()["loss"])
    eng.lbfgs_run(30)
    rel = max(abs(a - b) / abs(b) for a, b in zip(got, want))
    print(f"[whole run physics] worst relative loss deviation over 10 iterations {rel:.3e}; n_iter {eng.lbfgs_read()['n_iter']}")
    assert rel <= PHYS_TRAJ_TOL, (rel, got, want)
    assert eng.lbfgs_read()["n_iter"] == 40
    eng.close()


# measured once against the fp64 trajectory (profiles/lbfgs/trajectory.txt), times 4 for box-to-box and seed spread
MSE_TRAJ_TOL = 4 * 2.336e-06     # measured 2.336e-06 (losses 7.5 -> 3.1e-2 over the 10 iterations)
PHYS_TRAJ_TOL = 4 * 4.482e-07    # measured 4.482e-07 (losses 2059 -> 1820)


def test_refine_pretrain_device_tail(monkeypatch):
    from gpe_pinn import refine
    X = np.linspace(-10, 10, 512).reshape(-1, 1)
    losses = {}
    calls = {"n": 0}
    real = Engine.get_grad

    def counting(self):
        calls["n"] += 1
        return real(self)

    for how in ("host", "device"):
        torch.manual_seed(0)
        np.random.seed(0)
        model = refine.GrossPitaevskiiPINN([1, 32, 32, 1], mode=0, gamma=0.0)
        if how == "device":
            monkeypatch.setattr(Engine, "get_grad", counting)
        model = refine.pretrain_on_analytical_solution(model, 0, X, epochs=520, lr=1e-3, lbfgs=how) if how == "device" else \
            refine.pretrain_on_analytical_solution(model, 0, X, epochs=520, lr=1e-3)
        losses[how] = model.pretrain_loss
        model.close()
    print(f"[refine pretrain] host {losses['host']:.3e} device {losses['device']:.3e}")
    assert calls["n"] == 0
    assert losses["device"] <= 10.0 * losses["host"], losses


def test_refusals():
    layers, path = SHAPES["P1153"]
    eng = make_engine(layers, path)
    for call in (eng.lbfgs_update, lambda: eng.lbfgs_run(1), eng.lbfgs_read, eng.lbfgs_history):
        with pytest.raises(GPEError, match="not configured") as ei:
            call()
        assert ei.value.code == capi.GPE_ERR_STATE
    for bad in (dict(lr=0.1, history=0), dict(lr=0.1, history=129), dict(lr=float("nan")), dict(lr=-1.0), dict(lr=0.1, tolerance_grad=-1.0),
                dict(lr=0.1, tolerance_change=float("inf")), dict(lr=0.1, stop_loss=-1.0)):
        with pytest.raises(GPEError) as ei:
            eng.lbfgs_config(**bad)
        assert ei.value.code == capi.GPE_ERR_INVALID, bad
    eng.lbfgs_config(0.1, history=3)
    with pytest.raises(GPEError, match="without step_backward") as ei:
        eng.lbfgs_update()
    assert ei.value.code == capi.GPE_ERR_STATE
    with pytest.raises(GPEError) as ei:                                   # mse mode without a target
        eng.lbfgs_run(1, mse=True)
    assert ei.value.code == capi.GPE_ERR_STATE
    eng.bind_sampler([-3.0], [3.0], [N], every=2, seed=1)
    for call in (eng.lbfgs_update, lambda: eng.lbfgs_run(1)):
        with pytest.raises(GPEError, match="sampler") as ei:
            call()
        assert ei.value.code == capi.GPE_ERR_STATE
    eng.close()
    # gpe_comm_init done: update and run are refused, and so is a (re)configuration
    eng = make_engine(layers, path)
    eng.lbfgs_config(0.1, history=3)
    eng.comm_init(0, 1)
    eng.step_begin(); eng.step_backward()
    for call in (eng.lbfgs_update, lambda: eng.lbfgs_run(1)):
        with pytest.raises(GPEError, match="communicator") as ei:
            call()
        assert ei.value.code == capi.GPE_ERR_STATE
    with pytest.raises(GPEError, match="data-parallel") as ei:
        eng.lbfgs_config(0.1, history=3)
    assert ei.value.code == capi.GPE_ERR_INVALID
    eng.comm_destroy()
    eng.close()
    dp = Engine(GPEConfig(layers=layers, world_size=2))
    with pytest.raises(GPEError, match="data-parallel") as ei:
        dp.lbfgs_config(0.1)
    assert ei.value.code == capi.GPE_ERR_INVALID
    dp.close()
