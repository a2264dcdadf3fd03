"""The float64 update reference (oracle/update_ref.py) against independent implementations of the same operations: torch's own
clip_grad_norm_ + Adam + CosineAnnealingWarmRestarts.step(loss) / ReduceLROnPlateau in float64, and gpe_oracle.optimizer_step.  Its
agreement with them is what makes the GPU assertions of tests/test_gpu_update_kernel.py meaningful.

Tolerance: 1e-12 of the largest magnitude -- double round-off (1.1e-16) through ~40 steps of ~10 operations each, with head room for
torch's beta ** step against the running products kept here (<= 40 ulp at step 40).  No GPU."""
import math

import numpy as np
import pytest
import torch

from oracle import gpe_oracle as go
from oracle import update_ref as ur
from tests.update_scripts import COSINE_T1, COSINE_T2, PLATEAU, PLATEAU_KW, f32

P, STEPS = 200, 40
RTOL = 1e-12

def _inputs(seed=0, p=P):
    rng = np.random.default_rng(seed)
    theta = rng.normal(0, 1, p)
    grads = [rng.normal(0, 1, p) * 10.0 ** rng.uniform(-3, 1) for _ in range(STEPS)]      # norms on both sides of the clip
    return theta, grads


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err, scale = np.abs(a - b).max(), np.abs(b).max()
    assert err <= RTOL * scale, (what, err, scale)


def _torch_run(theta, grads, losses, sched, clip, lr=1e-3, **kw):
    p = torch.nn.Parameter(torch.tensor(theta, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=lr, foreach=False)
    if sched == ur.SCHED_COSINE_LOSS:
        sch = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=int(kw["T_0"]), T_mult=int(kw["T_mult"]), eta_min=kw["eta_min"])
    elif sched == ur.SCHED_PLATEAU:
        sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=kw["factor"], patience=kw["patience"], min_lr=kw["min_lr"],
                                                         threshold=kw["threshold"], threshold_mode="rel")
    else:
        sch = None
    out = []
    for g, loss in zip(grads, losses):
        p.grad = torch.tensor(g, dtype=torch.float64)
        lr_used = opt.param_groups[0]["lr"]
        gn = float(torch.nn.utils.clip_grad_norm_([p], clip)) if clip > 0 else float(p.grad.norm())
        opt.step()
        if sch is not None:
            sch.step(torch.tensor(loss, dtype=torch.float32).item() if sched == ur.SCHED_COSINE_LOSS else loss)
        st = opt.state[p]
        out.append(dict(theta=p.detach().numpy().copy(), m=st["exp_avg"].numpy().copy(), v=st["exp_avg_sq"].numpy().copy(), gn=gn, lr=lr_used))
    return out


@pytest.mark.parametrize("clip", [1.0, 0.0], ids=["clip1", "noclip"])
def test_clip_and_adam_against_torch(clip):
    theta, grads = _inputs(1)
    ref = ur.UpdateRef(theta, lr=1e-3, clip_norm=clip)
    tr = _torch_run(theta, grads, [1.0] * STEPS, ur.SCHED_CONST, clip)
    clipped = 0
    for k, g in enumerate(grads):
        r = ref.update(g, 1.0)
        assert r["status"] == "applied" and ref.step == k + 1
        clipped += r["coef"] < 1.0
        _close(r["theta"], tr[k]["theta"], f"theta step {k + 1}")
        _close(r["m"], tr[k]["m"], f"m step {k + 1}")
        _close(r["v"], tr[k]["v"], f"v step {k + 1}")
        _close(r["grad_norm"], tr[k]["gn"], "grad norm")
    assert (0 < clipped < STEPS) if clip > 0 else clipped == 0          # both branches of the clip ran


@pytest.mark.parametrize("T_mult,losses", [(2, COSINE_T2), (1, COSINE_T1)], ids=["T_mult2", "T_mult1"])
def test_cosine_on_loss_against_torch(T_mult, losses):
    """CosineAnnealingWarmRestarts.step(loss): the restart branches (loss >= T_0), T_mult = 1 included, eta_min > 0; the lr every step
    USED and the parameters it produced."""
    assert len(losses) == STEPS
    kw = dict(T_0=200.0, T_mult=float(T_mult), eta_min=1e-5)
    theta, grads = _inputs(2)
    ref = ur.UpdateRef(theta, lr=1e-3, sched=ur.SCHED_COSINE_LOSS, **kw)
    tr = _torch_run(theta, grads, losses, ur.SCHED_COSINE_LOSS, 1.0, **kw)
    for k, (g, loss) in enumerate(zip(grads, losses)):
        r = ref.update(g, loss)
        _close(r["lr"], tr[k]["lr"], f"lr used by step {k + 1}")
        _close(r["theta"], tr[k]["theta"], f"theta step {k + 1}")
    assert max(ur.cosine_cycle(f32(x), 200.0, float(T_mult))[0] for x in losses) >= 5


@pytest.mark.parametrize("T_mult,losses", [(2.0, COSINE_T2), (1.0, COSINE_T1)], ids=["T_mult2", "T_mult1"])
def test_scripted_losses_stay_clear_of_restart_boundaries(T_mult, losses):
    """At a restart boundary the lr jumps from eta_min to lr0: every scripted loss keeps its cycle (n, T_i) under a relative perturbation of
    1e-6, so that an fp32 engine fed the same script cannot land in another cycle by rounding -- and both sides of the boundaries at
    200, 600 / 400, 3000 / 1000 are there."""
    cycles = set()
    for x in losses:
        n, _, T_i = ur.cosine_cycle(f32(x), 200.0, T_mult)
        for s in (1 - 1e-6, 1 + 1e-6):
            n2, _, T2 = ur.cosine_cycle(f32(x) * s, 200.0, T_mult)
            assert (n2, T2) == (n, T_i), x
        cycles.add(n)
    assert {0, 1, 2}.issubset(cycles) and (T_mult == 1.0 or {3, 4, 8}.issubset(cycles)) and (T_mult == 2.0 or {4, 5, 500}.issubset(cycles))


def test_plateau_against_torch():
    """ReduceLROnPlateau: improvements just inside and just outside the relative threshold, three reductions of which the third clamps at
    min_lr, and a further bad run at the clamp (lr stays, the bad-epoch counter restarts)."""
    assert len(PLATEAU) == STEPS
    theta, grads = _inputs(3)
    ref = ur.UpdateRef(theta, lr=1e-3, sched=ur.SCHED_PLATEAU, **PLATEAU_KW)
    tr = _torch_run(theta, grads, PLATEAU, ur.SCHED_PLATEAU, 1.0, **PLATEAU_KW)
    lrs, bad = [], []
    for k, (g, loss) in enumerate(zip(grads, PLATEAU)):
        r = ref.update(g, loss)
        lrs.append(r["lr"])
        bad.append(ref.num_bad)
        _close(r["lr"], tr[k]["lr"], f"lr used by step {k + 1}")
        _close(r["theta"], tr[k]["theta"], f"theta step {k + 1}")
    assert bad[:7] == [0, 0, 1, 2, 3, 0, 0]                    # 0.99989 inside the threshold, 0.99980 outside; reduction resets
    assert sorted(set(lrs), reverse=True) == [1e-3, 5e-4, 2.5e-4, 2e-4]
    assert lrs.index(2e-4) == 15 and bad[18] == 0 and bad[23] == 0 and bad[27] == 0 and ref.lr == 2e-4      # the clamp, and two bad runs at it


@pytest.mark.parametrize("sched", [ur.SCHED_CONST, ur.SCHED_COSINE_LOSS, ur.SCHED_PLATEAU])
def test_against_the_existing_oracle_step(sched):
    """gpe_oracle.optimizer_step(dtype=float64) covers clip + Adam + both schedulers (no early stop, no skip): the two must agree there.
    (It takes the loss as the epoch unrounded, the reference here rounds it to fp32 first: the script is fed in fp32-exact values.)"""
    losses = [f32(x) for x in {ur.SCHED_CONST: [1.0] * STEPS, ur.SCHED_COSINE_LOSS: COSINE_T2, ur.SCHED_PLATEAU: PLATEAU}[sched]]
    theta, grads = _inputs(4)
    kw = dict(T_0=200.0, T_mult=2.0, eta_min=1e-5, **PLATEAU_KW)
    ref = ur.UpdateRef(theta, lr=1e-3, sched=sched, **kw)
    st = go.OptState(lr0=1e-3, sched=sched, **kw)
    flat = theta.copy()
    for g, loss in zip(grads, losses):
        r = ref.update(g, loss)
        flat, gn, lr_used = go.optimizer_step(st, flat, g, loss, dtype=np.float64)
        _close(r["theta"], flat, "theta")
        _close(r["grad_norm"], gn, "grad norm")
        _close(r["lr"], lr_used, "lr")
    assert ref.step == st.step == STEPS


def test_set_adam_state_bias_corrections():
    """A state set at step t continues exactly like t steps of running products would: ss = lr / (1 - beta1^(t+1)), sqrt(1 - beta2^(t+1))."""
    theta, grads = _inputs(5)
    rng = np.random.default_rng(6)
    m, v = rng.normal(0, 1e-2, P), rng.uniform(0, 1e-3, P)
    for t in (1, 1000, 100000):
        ref = ur.UpdateRef(theta, lr=1e-3)
        ref.set_adam_state(m, v, t)
        r = ref.update(grads[0], 1.0)
        assert ref.step == t + 1
        g = grads[0] * r["coef"]
        m1, v1 = 0.9 * m + (1 - 0.9) * g, 0.999 * v + (1 - 0.999) * g * g
        want = theta - 1e-3 / (1 - 0.9 ** (t + 1)) * m1 / (np.sqrt(v1) / math.sqrt(1 - 0.999 ** (t + 1)) + 1e-8)
        _close(r["theta"], want, f"theta from step {t}")


def test_early_stop_patience_and_freeze():
    """Best-loss counter: best at step 3, then three steps without a new best -> stop fires ON step 6, which is applied; afterwards nothing
    moves and the last record stays.  An equal loss is not a new best."""
    theta, grads = _inputs(7)
    ref = ur.UpdateRef(theta, lr=1e-3, stop_patience=3)
    losses = [5.0, 4.0, 3.0, 3.5, 3.0, 3.2, 0.1, 0.1]
    snaps = []
    for g, loss in zip(grads, losses):
        before = ref.theta.copy()
        r = ref.update(g, loss)
        snaps.append((r["status"], ref.step, ref.stopped, not np.array_equal(before, ref.theta)))
    assert snaps[:6] == [("applied", k + 1, k == 5, True) for k in range(6)]
    assert snaps[6:] == [("frozen", 6, True, False)] * 2
    assert (ref.stopped, ref.stop_step) == (True, 6) and ref.last["step"] == 6 and ref.last["loss"] == 3.2 and len(ref.history) == 6
    m, v = ref.m.copy(), ref.v.copy()
    ref.update(grads[0], 0.0)
    assert np.array_equal(m, ref.m) and np.array_equal(v, ref.v) and ref.step == 6
    ref.reset_optimizer(5e-4)                                  # a new optimiser: the stop is cleared, Adam starts over at step 1
    r = ref.update(grads[0], 9.0)
    assert r["status"] == "applied" and ref.step == 1 and not ref.stopped and r["lr"] == 5e-4 and ref.m.any()


def test_early_stop_tolerance():
    theta, grads = _inputs(8)
    ref = ur.UpdateRef(theta, lr=1e-3, stop_tol=1e-3, stop_patience=0)
    st = [ref.update(g, loss)["status"] for g, loss in zip(grads, [1.0, 0.1, 0.01, 1e-3, 1e-4, 1.0])]
    assert st == ["applied"] * 4 + ["frozen"] * 2 and (ref.stopped, ref.stop_step) == (True, 4)
    off = ur.UpdateRef(theta, lr=1e-3)                         # stop_tol = 0, stop_patience = 0: both tests disabled
    assert all(off.update(g, 0.0)["status"] == "applied" for g in grads[:5]) and not off.stopped


@pytest.mark.parametrize("bad", ["nan_grad", "inf_grad", "nan_loss", "inf_loss"])
def test_non_finite_is_skipped_and_sticky(bad):
    """No parameter, moment, step or beta-power change, no history record, a sticky flag; the next finite step is step k + 1."""
    theta, grads = _inputs(9)
    ref = ur.UpdateRef(theta, lr=1e-3, sched=ur.SCHED_PLATEAU, stop_patience=2, **PLATEAU_KW)
    twin = ur.UpdateRef(theta, lr=1e-3, sched=ur.SCHED_PLATEAU, stop_patience=2, **PLATEAU_KW)
    for r_ in (ref, twin):
        r_.update(grads[0], 2.0)
    g = grads[1].copy()
    loss = 1.0
    if bad.endswith("grad"):
        g[17] = np.nan if bad.startswith("nan") else np.inf
    else:
        loss = np.nan if bad.startswith("nan") else -np.inf
    state = (ref.theta.copy(), ref.m.copy(), ref.v.copy(), ref.step, ref.b1p, ref.b2p, ref.lr, ref.num_bad, ref.es_count, len(ref.history))
    assert ref.update(g, loss)["status"] == "skipped"
    after = (ref.theta, ref.m, ref.v, ref.step, ref.b1p, ref.b2p, ref.lr, ref.num_bad, ref.es_count, len(ref.history))
    assert all(np.array_equal(a, b) for a, b in zip(state, after))
    assert ref.nonfinite and ref.last["nonfinite"]
    a, b = ref.update(grads[2], 1.5), twin.update(grads[2], 1.5)           # the twin never saw the bad step
    assert ref.step == twin.step == 2 and np.array_equal(a["theta"], b["theta"]) and ref.nonfinite and not ref.last["nonfinite"]


def test_mse_mode_is_plain_adam():
    """Pre-training: no clip (a gradient of norm 50 is applied whole), no scheduler step, no early-stop bookkeeping."""
    theta, grads = _inputs(10)
    ref = ur.UpdateRef(theta, lr=1e-3, sched=ur.SCHED_COSINE_LOSS, stop_tol=1.0, stop_patience=1)
    plain = ur.UpdateRef(theta, lr=1e-3, clip_norm=0.0)
    for k in range(5):
        g = grads[k] * (50.0 / np.linalg.norm(grads[k]))
        a, b = ref.update(g, 0.5, mse_mode=True), plain.update(g, 0.5)
        assert a["coef"] == 1.0 and a["lr"] == 1e-3 and np.array_equal(a["theta"], b["theta"])
    assert not ref.stopped and ref.es_count == 0 and ref.step == 5 and len(ref.history) == 5
