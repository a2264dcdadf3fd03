"""The update kernel alone (update_core in csrc/gpe_update.h: gradient-norm clipping, Adam in torch's op order, bias-correction powers,
both schedulers, early stop, non-finite skip, history ring, packed-weight scatter) against the float64 reference oracle/update_ref.py,
which tests/test_update_reference_cpu.py holds to torch's own optimiser and schedulers.

Injection: between step_backward() and step_update() the update reads its gradient from Engine.exchange_grad ([P + 4] fp32) and the
residual sum from the tail element exchange_grad[P]; with w_pde = 1 and every other weight 0 the recorded loss is tail / n_global.  With
N = 256 points loss = tail / 256 is exact in fp32, so gradient AND loss of a step are whatever the test writes there; the batch only
satisfies the phase machine.

Bounds.  The reference is fed the engine's own fp32 state (theta, m, v read back before the step) and the same fp32 gradient, so one
step's difference is the round-off of the kernel's nine fp32 operations (g = graw coef; m += (g - m)(1 - b1); v = v b2 + ((1 - b2) g) g;
denom = sqrt(v) / b2s + eps; theta -= ss (m / denom)).  First-order propagation with unit round-off u = 2^-24 and a safety factor 2:
    |dm|     <= 2 * 3u (|g coef| + |m_old|)          (product, difference, product, sum: each term bounded by |g coef| + |m_old|)
    |dv|     <= 2 * 4u v_new                         (g carries u, g^2 2u, two products, the sum)
    |dtheta| <= 2 * [u |theta_new| + 6u |upd| + ss dm_bound / denom]
                                                     (final difference; sqrt, two quotients, sum, rounded ss and b2s, product;  m's error)
No tolerance here was measured on the GPU.  grad_norm: 1e-10 relative against the float64 sum (double accumulation of <= 33 537 terms is
good to 4e-12); lr of a scheduler step: 1e-12 relative (both sides evaluate the same double formula; device cos / log / pow are within a
few ulp and the scripts stay clear of the restart boundaries, which the CPU test asserts); lr, step, loss and pde otherwise exact.
"""
import os

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import GPEConfig, Engine, GPEError
from oracle import gpe_oracle as go
from oracle import update_ref as ur
from tests.update_scripts import COSINE_T1, COSINE_T2, PLATEAU, PLATEAU_KW, f32

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N = 256

# (layers, environment, path): every form of the injectable update at its edges
ROWS = {
    "cached_P1153": ([1, 32, 32, 1], {}, gpe_pinn.PATH_AUTO),                              # partial first register slot, P % 4 = 1
    "cached_P12737": ([2, 64, 64, 64, 64, 1], {}, gpe_pinn.PATH_AUTO),                     # last of the 13 register slots partly filled
    "twopass_P17025": ([2, 128, 128, 1], {}, gpe_pinn.PATH_AUTO),                          # one workgroup, two passes, gather repack
    "multi_P33537": ([2, 128, 128, 128, 1], {}, gpe_pinn.PATH_AUTO),                       # 64 workgroups, last chunk ragged (528)
    "multi_forced_P1153": ([1, 32, 32, 1], {"GPE_UPDATE_MULTI_MIN": "1"}, gpe_pinn.PATH_AUTO),   # 58 x 20 > P: trailing EMPTY workgroups
    "twopass_forced_P12737": ([2, 64, 64, 64, 64, 1], {"GPE_UPDATE_CACHE": "0"}, gpe_pinn.PATH_AUTO),
    "generic_P1153": ([1, 32, 32, 1], {}, gpe_pinn.PATH_GENERIC),                          # no packed copies
}
OPT_KEYS = ("lr", "beta1", "beta2", "eps", "clip_norm", "sched", "T_0", "T_mult", "eta_min", "factor", "patience", "min_lr", "threshold",
            "stop_tol", "stop_patience")


def make_engine(layers, env=None, path=gpe_pinn.PATH_AUTO, **kw):
    """Engine whose recorded loss is exactly tail / 256, on 256 fixed points; environment switches only around the constructor."""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine(GPEConfig(layers=layers, w_pde=1.0, w_bc=0.0, w_norm=0.0, w_sym=0.0, w_orth=0.0, w_riesz=0.0, dx=1.0, path=path, **kw))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    rng = np.random.default_rng(5)
    eng.bind_points(torch.as_tensor(rng.uniform(-3, 3, (N, layers[0])).astype(np.float32), device="cuda"))
    assert eng.exchange_grad.numel() == eng.n_params + 4 == go.param_count(layers) + 4
    return eng


def ref_for(eng, **over):
    """The float64 reference on the engine's optimiser settings as the engine holds them: rounded to fp32."""
    kw = {k: getattr(eng.cfg, k) for k in OPT_KEYS}
    kw.update(over)
    kw = {k: (v if isinstance(v, (int, np.integer)) and k in ("sched", "patience", "stop_patience") else f32(v)) for k, v in kw.items()}
    return ur.UpdateRef(eng.get_params(), **kw)


def inject(eng, g, loss):
    """One step whose update sees the gradient g and the loss float32(256 loss) / 256; returns that loss."""
    P = eng.n_params
    tail = np.float32(loss * N)
    buf = np.zeros(P + 4, np.float32)
    buf[:P] = g
    buf[P] = tail
    eng.step_begin()
    eng.step_backward()
    eng.synchronize()
    eng.exchange_grad.copy_(torch.as_tensor(buf, device="cuda"))
    torch.cuda.synchronize()
    eng.step_update()
    eng.synchronize()
    return float(tail) / N


def state(eng):
    m, v, step = eng.get_adam_state()
    return eng.get_params(), m, v, step


def check_elements(st1, r, m0, what):
    """theta, m, v after the step against the reference's, element by element, within the bounds of the module docstring."""
    th, m, v, _ = st1
    bm = 2 * 3 * U * (np.abs(r["g"]) + np.abs(m0))
    bv = 2 * 4 * U * r["v"]
    bt = 2 * (U * np.abs(r["theta"]) + 6 * U * np.abs(r["upd"]) + r["ss"] * bm / r["denom"])
    for name, got, want, bound in (("m", m, r["m"], bm), ("v", v, r["v"], bv), ("theta", th, r["theta"], bt)):
        err = np.abs(got.astype(np.float64) - want)
        ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
        i = int(np.argmax(ratio))
        print(f"[{what}] {name}: worst err/bound {ratio[i]:.3f} at element {i} (err {err[i]:.3e}, bound {bound[i]:.3e})")
        assert (err <= bound).all(), (what, name, i, float(err[i]), float(bound[i]), float(got[i]), float(want[i]))


def synced_step(eng, ref, g, loss, what, mse=False):
    """Hand the reference the engine's fp32 state, inject one step into both, compare.  Returns (record or None, reference result)."""
    th0, m0, v0, step0 = state(eng)
    ref.theta, ref.m, ref.v = th0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    assert step0 == ref.step, what
    loss_in = inject(eng, g, loss)
    r = ref.update(np.asarray(g, np.float32), loss_in)
    st1 = state(eng)
    assert st1[3] == ref.step, (what, st1[3], ref.step)
    if r["status"] != "applied":
        for a, b in zip(st1[:3], (th0, m0, v0)):
            np.testing.assert_array_equal(a, b, err_msg=what)                 # bitwise: nothing moved
        return None, r
    rec = eng.read_scalars()
    gn64 = float(np.sqrt((np.asarray(g, np.float32).astype(np.float64) ** 2).sum()))
    assert abs(rec["grad_norm"] - gn64) <= 1e-10 * gn64, (what, rec["grad_norm"], gn64)
    assert rec["loss"] == loss_in and rec["pde"] == loss_in and rec["step"] == ref.step and rec["nonfinite"] == 0.0, (what, rec, loss_in)
    assert abs(rec["lr"] - r["lr"]) <= 1e-12 * r["lr"], (what, rec["lr"], r["lr"])
    check_elements(st1, r, m0.astype(np.float64), what)
    return rec, r


def random_state(P, seed):
    rng = np.random.default_rng(seed)
    theta = rng.normal(0, 0.3, P).astype(np.float32)
    m = (rng.normal(0, 1, P) * 10.0 ** rng.uniform(-6, -1, P)).astype(np.float32)
    v = (10.0 ** rng.uniform(-16, 0, P)).astype(np.float32)
    return theta, m, v, rng


def wide_gradient(P, rng, top=3.0):
    return (rng.choice([-1.0, 1.0], P) * 10.0 ** rng.uniform(-12, top, P)).astype(np.float32)


def scaled_to(g, norm):
    g = g.astype(np.float64)
    return (g * (norm / np.sqrt((g * g).sum()))).astype(np.float32)


@pytest.mark.parametrize("row", list(ROWS))
def test_elementwise_against_reference(row):
    """Every injectable form of the update, from states set with set_params / set_adam_state: gradients over 15 decades with mixed signs
    and tiny clip factors; elements with g = m = v = 0 (must not move); the all-zero gradient (|g| = 0, coef = 1: theta bitwise unchanged
    where m = 0); |g| = 1 exactly (coef = 1 / (1 + 1e-6), not 1: m shows it, 17 fp32 ulps against a bound of 6); |g| = 0.5 (no clipping);
    |g| ~ 1e3; bias corrections at steps 1, 1 000 and 100 000 (set_adam_state sets the beta powers by pow)."""
    layers, env, path = ROWS[row]
    eng = make_engine(layers, env, path)
    assert eng.active_path == (gpe_pinn.PATH_GENERIC if path == gpe_pinn.PATH_GENERIC else gpe_pinn.PATH_FUSED)
    P = eng.n_params
    theta, m, v, rng = random_state(P, 11)
    dead = np.arange(3, P, 7)
    m[dead] = 0.0
    v[dead] = 0.0

    def case(what, g, m_, v_, step):
        eng.set_params(theta)
        eng.set_adam_state(m_, v_, step)
        ref = ref_for(eng)
        ref.set_adam_state(m_, v_, step)
        rec, r = synced_step(eng, ref, g, 0.75, f"{row}/{what}")
        assert rec is not None and rec["lr"] == f32(1e-3)
        return r

    g = wide_gradient(P, rng)
    g[dead] = 0.0
    r = case("wide", g, m, v, 7)
    assert r["coef"] < 1e-2
    np.testing.assert_array_equal(eng.get_params()[dead], theta[dead])
    ma, va, _ = eng.get_adam_state()
    assert not ma[dead].any() and not va[dead].any()

    zero_m = np.zeros(P, np.float32)
    r = case("zero_gradient", np.zeros(P, np.float32), zero_m, v, 7)
    assert r["grad_norm"] == 0.0 and r["coef"] == 1.0 and eng.read_scalars()["grad_norm"] == 0.0
    np.testing.assert_array_equal(eng.get_params(), theta)

    one = np.zeros(P, np.float32)
    one[P // 2] = 1.0
    r = case("unit_norm", one, zero_m, v, 7)
    assert r["grad_norm"] == 1.0 and r["coef"] == 1.0 / (1.0 + 1e-6)
    assert eng.get_adam_state()[0][P // 2] == np.float32(np.float32(r["coef"]) * np.float32(1.0 - np.float32(0.9)))

    r = case("norm_half", scaled_to(wide_gradient(P, rng, top=0.0), 0.5), m, v, 7)
    assert r["coef"] == 1.0
    r = case("norm_1e3", scaled_to(rng.normal(0, 1, P), 1e3), m, v, 7)
    assert abs(r["coef"] - 1e-3) < 1e-8
    gmid = scaled_to(rng.normal(0, 1, P), 3.0)
    for step in (1, 1000, 100000):
        case(f"from_step_{step}", gmid, m, v, step)
    eng.close()


@pytest.mark.parametrize("row", list(ROWS))
def test_no_clipping_with_huge_gradients(row):
    """clip_norm = 0: |g| up to 1e6 goes into the moments unscaled."""
    layers, env, path = ROWS[row]
    eng = make_engine(layers, env, path, clip_norm=0.0)
    P = eng.n_params
    theta, m, v, rng = random_state(P, 12)
    eng.set_params(theta)
    eng.set_adam_state(m, v, 3)
    ref = ref_for(eng)
    ref.set_adam_state(m, v, 3)
    rec, r = synced_step(eng, ref, wide_gradient(P, rng, top=6.0), 2.0, row)
    assert r["coef"] == 1.0 and rec["grad_norm"] > 1e6
    eng.close()


def small_gradient(P, seed=21):
    return scaled_to(np.random.default_rng(seed).normal(0, 1, P), 0.3)


@pytest.mark.parametrize("name,kw,losses", [
    ("cosine_T_mult2", dict(sched=go.SCHED_COSINE_LOSS, T_0=200.0, T_mult=2.0, eta_min=1e-5), COSINE_T2),
    ("cosine_T_mult1", dict(sched=go.SCHED_COSINE_LOSS, T_0=200.0, T_mult=1.0, eta_min=1e-5), COSINE_T1),
    ("plateau", dict(sched=go.SCHED_PLATEAU, **PLATEAU_KW), PLATEAU)], ids=lambda a: a if isinstance(a, str) else "")
def test_scheduler_scripts(name, kw, losses):
    """40 injected steps of scripted losses: cosine-on-loss through the restart branches (n = int(log / log), T_cur, T_i; the fmod branch of
    T_mult = 1; eta_min > 0), plateau with an improvement just inside and one just outside the relative threshold, three reductions of
    which the third clamps at min_lr, and bad runs at the clamp.  The lr every step records (the one it used), its loss and step, and the
    elements of every step, against the reference."""
    layers = [1, 32, 32, 1]
    eng = make_engine(layers, lr=1e-3, **kw)
    eng.set_params(np.random.default_rng(1).normal(0, 0.3, eng.n_params).astype(np.float32))
    ref = ref_for(eng)
    g = small_gradient(eng.n_params)
    lrs = []
    for k, loss in enumerate(losses):
        rec, _ = synced_step(eng, ref, g, loss, f"{name} step {k + 1}")
        lrs.append(rec["lr"])
    hist = eng.read_history(1, len(losses))
    assert [h["lr"] for h in hist] == lrs and [h["step"] for h in hist] == list(range(1, len(losses) + 1))
    assert len(set(lrs)) >= (4 if name == "plateau" else 20)          # (the schedule moved: T_mult = 1 maps 199, 399, 599 to one lr)
    if name == "plateau":
        assert lrs[-1] == f32(2e-4) and sorted(set(lrs))[1] == f32(1e-3) / 4
    assert eng.stop_state() == (False, 0)
    eng.close()


@pytest.mark.parametrize("kw,losses,stop_at", [(dict(stop_patience=3, stop_tol=0.0), [5.0, 4.0, 3.0, 3.5, 3.0, 3.2], 6),
                                               (dict(stop_patience=0, stop_tol=1e-3), [1.0, 0.1, 0.01, 1e-3], 4)], ids=["patience", "tolerance"])
def test_early_stop_and_frozen_state(kw, losses, stop_at):
    """The stop fires at the reference's step (patience: best at step 3, an EQUAL loss at step 5 is no new best; tolerance: loss == stop_tol
    counts), that step is applied, and afterwards theta, m, v and step stay bitwise, the last record stays the stop step's and the history
    slot behind it stays zero.  reset_optimizer clears the stop: the next step is step 1."""
    eng = make_engine([1, 32, 32, 1], lr=1e-3, **kw)
    eng.set_params(np.random.default_rng(2).normal(0, 0.3, eng.n_params).astype(np.float32))
    ref = ref_for(eng)
    g = small_gradient(eng.n_params)
    for k, loss in enumerate(losses):
        assert eng.stop_state() == (False, 0)
        before = eng.get_params()
        rec, _ = synced_step(eng, ref, g, loss, f"step {k + 1}")
        assert rec is not None
    assert ref.stopped and ref.stop_step == stop_at == len(losses)
    assert eng.stop_state() == (ref.stopped, ref.stop_step)
    assert (eng.get_params() != before).any()                         # the stopping step itself moved the parameters
    frozen, last = state(eng), eng.read_scalars()
    assert last["step"] == stop_at
    for k in range(5):
        rec, r = synced_step(eng, ref, small_gradient(eng.n_params, 30 + k), 0.5 * losses[-1], f"frozen {k + 1}")
        assert rec is None and r["status"] == "frozen"
    for a, b in zip(state(eng), frozen):
        np.testing.assert_array_equal(a, b)
    assert eng.read_scalars() == last and eng.stop_state() == (True, stop_at)
    assert all(val == 0.0 for val in eng.read_history(stop_at + 1, 1)[0].values())
    eng.reset_optimizer(5e-4)
    ref.reset_optimizer(f32(5e-4))
    assert eng.stop_state() == (False, 0)
    rec, r = synced_step(eng, ref, g, 9.0, "after reset")
    assert rec["step"] == 1 and rec["lr"] == f32(5e-4) and eng.stop_state() == (False, 0)
    eng.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_non_finite_gradient_with_finite_loss_is_skipped(bad):
    """One non-finite gradient element, finite loss: theta, m, v bitwise unchanged, step not advanced, read_scalars raises
    GPE_ERR_NONFINITE; the next finite step is the reference's step k + 1 -- the beta powers did not advance on the skipped one."""
    eng = make_engine([1, 32, 32, 1], lr=1e-3)
    eng.set_params(np.random.default_rng(3).normal(0, 0.3, eng.n_params).astype(np.float32))
    ref = ref_for(eng)
    g = small_gradient(eng.n_params)
    for k in range(2):
        synced_step(eng, ref, g, 1.0, f"step {k + 1}")
    gb = g.copy()
    gb[17] = bad
    rec, r = synced_step(eng, ref, gb, 1.0, "bad step")                # (asserts bitwise theta, m, v and the step count)
    assert rec is None and r["status"] == "skipped" and eng.get_adam_state()[2] == 2
    with pytest.raises(GPEError) as ei:
        eng.read_scalars()
    assert ei.value.code == gpe_pinn.capi.GPE_ERR_NONFINITE
    rec, r = synced_step(eng, ref, g, 1.0, "step after the skipped one")
    assert rec["step"] == 3 and abs(r["ss"] - f32(1e-3) / (1 - f32(0.9) ** 3)) < 1e-15
    assert [h["step"] for h in eng.read_history(1, 3)] == [1, 2, 3]
    eng.close()


def test_history_ring_wraps():
    """history_capacity = 8: after 20 steps the ring holds steps 13 .. 20 in order (slot (step - 1) % 8); a window larger than the ring is
    refused.  Once with injected steps (distinct losses), once with run(20) on real gradients, whose captured-graph replays write the ring."""
    eng = make_engine([1, 32, 32, 1], lr=1e-3, history_capacity=8)
    eng.set_params(np.random.default_rng(4).normal(0, 0.3, eng.n_params).astype(np.float32))
    g = small_gradient(eng.n_params)
    losses = [inject(eng, g, 0.5 * (k + 1)) for k in range(20)]
    hist = eng.read_history(13, 8)
    assert [h["step"] for h in hist] == list(range(13, 21)) and [h["loss"] for h in hist] == losses[12:]
    with pytest.raises(GPEError) as ei:
        eng.read_history(1, 9)
    assert ei.value.code == gpe_pinn.capi.GPE_ERR_INVALID
    eng.close()
    eng = Engine(GPEConfig(layers=[1, 32, 32, 1], w_bc=0.0, dx=16.0 / N, lr=1e-3, history_capacity=8))
    eng.set_params(np.random.default_rng(4).normal(0, 0.3, eng.n_params).astype(np.float32))
    eng.bind_points(torch.as_tensor(np.linspace(-8, 8, N, dtype=np.float32).reshape(-1, 1), device="cuda"))
    eng.run(20)
    hist = eng.read_history(13, 8)
    assert [h["step"] for h in hist] == list(range(13, 21)) and eng.read_scalars() == hist[-1]
    assert len({h["loss"] for h in hist}) == 8
    eng.close()


def test_mse_mode_is_plain_adam():
    """Pre-training step from a set Adam state: the engine's own gradient (get_grad) applied with coef = 1 although its norm is far above
    clip_norm, no scheduler step (cosine configured: a second step still records lr0), no early-stop bookkeeping (stop_tol above the loss)."""
    layers = [1, 32, 32, 1]
    eng = make_engine(layers, lr=1e-3, sched=go.SCHED_COSINE_LOSS, eta_min=1e-5, stop_tol=1e9)
    P = eng.n_params
    theta, m, v, rng = random_state(P, 13)
    eng.set_params(theta)
    eng.set_adam_state(m, v, 5)
    eng.bind_target(torch.as_tensor((10.0 + rng.normal(0, 1, (N, 1))).astype(np.float32), device="cuda"))
    ref = ref_for(eng)
    ref.set_adam_state(m, v, 5)
    for k in range(2):
        th0, m0, v0, step0 = state(eng)
        ref.theta, ref.m, ref.v = th0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
        rec = eng.mse_step()
        g = eng.get_grad()
        r = ref.update(g, rec["loss"], mse_mode=True)
        assert r["coef"] == 1.0 and r["grad_norm"] > 2.0
        assert rec["lr"] == f32(1e-3) and rec["step"] == 6 + k and abs(rec["grad_norm"] - r["grad_norm"]) <= 1e-10 * r["grad_norm"]
        check_elements(state(eng), r, m0.astype(np.float64), f"mse step {k + 1}")
    assert eng.stop_state() == (False, 0)
    eng.close()


def forward_matches_fresh_engine(eng, layers):
    """The packed MFMA copies the update scattered / repacked hold exactly the parameters: forward bitwise equal to a fresh engine's."""
    x = torch.as_tensor(np.random.default_rng(8).uniform(-3, 3, (64, layers[0])).astype(np.float32), device="cuda")
    fresh = Engine(eng.cfg)
    fresh.set_params(eng.get_params())
    a, b = eng.forward(x).cpu().numpy(), fresh.forward(x).cpu().numpy()
    fresh.close()
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("layers", [[1, 32, 32, 32, 32, 1], [2, 64, 64, 64, 64, 1]], ids=["1d_32x4", "2d_64x4"])
@pytest.mark.parametrize("env", [{}, {"GPE_FUSE_UPDATE": "1"}, {"GPE_SPLIT_UPDATE": "1"}], ids=["default", "fuse_update", "split_update"])
def test_whole_step_forms(layers, env):
    """The update inside the slab-reduction launch (k_reduce_update) and the split update exist only inside step(): six whole steps, each
    checked by applying the reference update to the engine's OWN gradient and recorded loss (the gradient is the update's input here;
    parity proper tests it) -- same bounds; the cosine scheduler's lr of the next step; and at the end the packed copies."""
    d = layers[0]
    n = 700
    rng = np.random.default_rng(3)
    x = (np.linspace(-8, 8, n).reshape(-1, 1) if d == 1 else rng.uniform(-4, 4, (n, d))).astype(np.float32)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine(GPEConfig(layers=layers, gamma=1.0, p=3, base_mode=0 if d == 1 else -1, base_deriv=1, dx=16.0 / n, lr=1e-3,
                               sched=go.SCHED_COSINE_LOSS, eta_min=1e-5))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    eng.set_params(rng.normal(0, 0.3, eng.n_params).astype(np.float32))
    eng.bind_points(torch.as_tensor(x, device="cuda"))
    if d == 1:
        eng.bind_boundary(torch.tensor([[-8.0], [8.0]], device="cuda"))
    ref = ref_for(eng)
    for k in range(6):
        th0, m0, v0, step0 = state(eng)
        ref.theta, ref.m, ref.v = th0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
        assert step0 == k == ref.step
        rec = eng.step()
        g = eng.get_grad()
        r = ref.update(g, rec["loss"])
        assert r["status"] == "applied" and rec["step"] == k + 1
        assert abs(rec["grad_norm"] - r["grad_norm"]) <= 1e-10 * r["grad_norm"]
        assert abs(rec["lr"] - r["lr"]) <= 1e-12 * r["lr"], (k, rec["lr"], r["lr"])
        check_elements(state(eng), r, m0.astype(np.float64), f"step {k + 1}")
    forward_matches_fresh_engine(eng, layers)
    eng.close()


def test_deferred_repack_after_multi_workgroup_update():
    """The multi-workgroup update leaves the repack of the hidden-hidden weights to the next k_begin: a forward straight after an injected
    update must already see the new weights."""
    layers = [2, 128, 128, 128, 1]
    eng = make_engine(layers, lr=1e-3)
    eng.set_params(np.random.default_rng(6).normal(0, 0.3, eng.n_params).astype(np.float32))
    before = eng.get_params()
    inject(eng, scaled_to(np.random.default_rng(7).normal(0, 1, eng.n_params), 5.0), 1.0)
    assert (eng.get_params() != before).all()
    forward_matches_fresh_engine(eng, layers)
    eng.close()
