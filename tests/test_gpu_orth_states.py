"""Frozen orthogonality states (include/gpe_hip.h: gpe_bind_orth_state / gpe_orth_values): psi_k evaluated by the engine itself from a
frozen parameter set of its own network, on every collocation set it holds -- against the fp64 oracle per forward-kernel family, as a
drop-in for a caller array in the step, through the sampler's redraws, under later setters, on two halves of a grid, and its refusals.

The frozen parameters always come from another seed than the engine's own: reading the trained parameters by mistake fails."""
import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import capi
from gpe_pinn.sampler import stratified_points
from oracle import gpe_oracle as go
from tests import helpers as H
from tests.test_gpu_parity import PATHS, _inputs, _scale, close, make_engine

pytestmark = pytest.mark.gpu


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _frozen(kw, seed=1):
    """a parameter set of the network of kw from another seed than _inputs' (0)"""
    rng = np.random.default_rng(1000 + seed)
    return (rng.normal(0, 1, go.param_count(kw["layers"], kw.get("net_kind", 0))) * _scale(kw)).astype(np.float32)


def _oracle_psi(kw, theta, x, base_mode=-1, perturb_scale=1.0, amplitude=1.0):
    """amplitude * (env * perturb_scale * NN_theta + phi_base_mode) in fp64"""
    pb = go.Problem(**{**kw, "base_mode": base_mode})
    _, skip, plain = go.expand_layers(pb.layers, pb.net_kind)
    x64 = np.asarray(x, np.float64)
    out, _ = go.mlp_forward(go.unflatten(theta.astype(np.float64), pb.layers, pb.net_kind), x64, pb.activation, value_only=True,
                            skip=skip, plain_tanh=plain)
    v = perturb_scale * out[0, :, 0]
    if pb.envelope == go.ENV_SIN:
        v = v * go.envelope(pb, x64[:, 0])[0]
    if base_mode >= 0:
        v = v + go.base_functions(pb, x64[:, 0])[0]
    return amplitude * v


def _state(eng):
    m, v, step = eng.get_adam_state()
    return eng.get_params(), m, v, step


def _same_state(a, b):
    return all(_same_bits(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]


def _raises(code, fn, *args, **kw):
    with pytest.raises(gpe_pinn.GPEError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, (ei.value.code, str(ei.value))


# ---- 1. values against the fp64 oracle, one case per forward-kernel family ---------------------------------------------------------
VALUE_CASES = {
    # name: (Problem kwargs, N, path, frozen base_mode, frozen perturb_scale)
    "1d_64x3_base": (dict(layers=[1, 64, 64, 64, 1], gamma=3.0, base_mode=2, dx=12 / 799), 800, "fused", 0, 0.37),
    "2d_64x4": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=36 / 2000), 2000, "fused", -1, 1.0),
    "2d_64x4_N17_ragged": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=36 / 17), 17, "fused", -1, 1.0),
    "2d_128x3": (dict(layers=[2, 128, 128, 128, 1], gamma=50.0, dx=36 / 500), 500, "fused", -1, 1.0),
    "2d_100x3_padded": (dict(layers=[2, 100, 100, 100, 1], gamma=50.0, dx=36 / 300), 300, "fused", -1, 1.0),
    "3d_256x2": (dict(layers=[3, 256, 256, 1], gamma=20.0, dx=0.01, omega=(1.0, 1.4, 2.0)), 300, "fused", -1, 1.0),
    "1d_residual_64x2blocks": (dict(layers=[1, 64, 64, 64, 1], net_kind=go.NET_RESIDUAL, gamma=2.0, dx=12 / 332), 333, "generic", -1, 1.0),
    "2d_residual_64x2blocks": (dict(layers=[2, 64, 64, 64, 1], net_kind=go.NET_RESIDUAL, gamma=20.0, dx=0.01), 300, "fused", -1, 1.0),
    "2d_64x3_generic": (dict(layers=[2, 64, 64, 64, 1], gamma=50.0, dx=0.01), 300, "generic", -1, 1.0),
}


@pytest.mark.parametrize("name", sorted(VALUE_CASES))
def test_values_match_the_fp64_oracle(name):
    kw, N, path, base_mode, s = VALUE_CASES[name]
    x, flat, _ = _inputs(kw, N, scale=_scale(kw))
    theta = _frozen(kw)
    eng = make_engine(go.Problem(**kw), flat, x, path=PATHS[path])
    assert eng.active_path == PATHS[path]
    eng.bind_orth_state(0, theta, base_mode=base_mode, perturb_scale=s)
    v1 = eng.orth_values(0)
    assert tuple(v1.shape) == (N,) and v1.dtype == torch.float32
    ref = _oracle_psi(kw, theta, x, base_mode, s)
    assert close(v1.cpu().numpy(), ref, 5e-6, 2e-6), float(np.abs(v1.cpu().numpy() - ref).max())
    assert not close(v1.cpu().numpy(), _oracle_psi(kw, flat, x, base_mode, s), 1e-3, 1e-3)      # (the trained parameters give something else)
    eng.bind_orth_state(0, theta, base_mode=base_mode, perturb_scale=s, amplitude=2.0)
    assert _same_bits(eng.orth_values(0), 2.0 * v1)
    eng.close()


# ---- 2. a frozen state is a drop-in for the caller array of its values; the step against the oracle ---------------------------------
def test_step_identity_with_caller_arrays_and_oracle_parity():
    kw, N = dict(layers=[1, 64, 64, 64, 1], gamma=3.0, base_mode=2, w_orth=7.0, dx=12 / 799), 800
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    states = [(_frozen(kw, 1), 0, 0.37, 1.0), (_frozen(kw, 2), 1, 0.5, 0.8)]
    a = make_engine(pb, flat, x, x_bc, sched=capi.SCHED_CONST)
    b = make_engine(pb, flat, x, x_bc, sched=capi.SCHED_CONST)
    for j, (th, bm, s, amp) in enumerate(states):
        a.bind_orth_state(j, th, base_mode=bm, perturb_scale=s, amplitude=amp)
    vals = [a.orth_values(j) for j in range(2)]
    for j in range(2):
        b.bind_orth(j, vals[j])
    orth64 = np.stack([v.cpu().numpy().astype(np.float64) for v in vals])
    osc, ograd, _ = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64), orth=orth64)
    assert osc["orth"] > 1e-4 * osc["loss"]            # the term matters in this case
    sc = a.step()
    b.step()
    for k, tol in (("mu", 2e-5), ("loss", 1e-4), ("orth", 1e-4), ("pde", 1e-4)):
        assert abs(sc[k] - osc[k]) <= tol * max(abs(osc[k]), 1e-6), (k, sc[k], osc[k])
    assert H.rel_err(a.get_grad(), ograd) < 5e-5
    for _ in range(2):
        a.step(); b.step()
    assert _same_state(_state(a), _state(b)) and _state(a)[3] == 3
    assert _same_bits(a.get_grad(), b.get_grad())
    for j in range(2):                                   # ... and the steps left the frozen values alone
        assert _same_bits(a.orth_values(j), vals[j])
    a.close(); b.close()


# ---- 3. sampler + frozen state == host loop of bind_points + bind_orth ---------------------------------------------------------------
@pytest.mark.parametrize("side,every", [(64, 5), (192, 5)], ids=["graph_every5", "above_graph_threshold"])
def test_sampler_trajectory_equals_host_loop(side, every):
    kw = dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, w_orth=3.0, dx=36.0 / (side * side))
    _, flat, x_bc = _inputs(kw, 100)
    pb = go.Problem(**kw)
    theta = _frozen(kw)
    g = dict(lo=(-3.0, -3.0), hi=(3.0, 3.0), shape=(side, side), seed=4242)
    steps = 3 * every + 2
    a = make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc, sched=capi.SCHED_CONST)
    a.bind_orth_state(0, theta, amplitude=0.7)
    a.bind_sampler(every=every, **g)
    a.run(steps)
    b = make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc, sched=capi.SCHED_CONST)
    helper = make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc)
    helper.bind_orth_state(0, theta, amplitude=0.7)
    done = 0
    for m in range(4):
        pts = torch.as_tensor(stratified_points(draw=m, **g), device="cuda")
        helper.bind_points(pts)
        b.bind_orth(0, None)
        b.bind_points(pts)
        b.bind_orth(0, helper.orth_values(0))
        k = min(every, steps - done)
        b.run(k)
        done += k
    assert done == steps
    sa, sb = _state(a), _state(b)
    assert sa[3] == steps
    assert _same_state(sa, sb), "sampler + frozen state differs from the host loop of bind_points + bind_orth"
    ha = a.read_history(1, steps)
    assert all(h["orth"] > 0 for h in ha)
    pts, draw = a.sampler_points()
    assert draw == 3
    helper.bind_points(pts)
    assert _same_bits(a.orth_values(0), helper.orth_values(0))
    a.close(); b.close(); helper.close()


# ---- 4. frozen means frozen ---------------------------------------------------------------------------------------------------------
def test_later_setters_leave_the_state_alone_rebinds_refill_and_clearing_restores_the_plain_step():
    kw, N = dict(layers=[1, 64, 64, 64, 1], gamma=3.0, base_mode=2, w_orth=7.0, dx=12 / 799), 800
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    theta = _frozen(kw)
    eng = make_engine(pb, flat, x, x_bc)
    eng.bind_orth_state(0, theta, base_mode=0, perturb_scale=0.37)
    v0 = eng.orth_values(0)
    eng.set_params(_frozen(kw, 5))
    eng.set_perturb_scale(0.11)
    eng.set_gamma(17.0)
    eng.reset_optimizer(3e-3)
    eng.step()
    assert _same_bits(eng.orth_values(0), v0)
    # another point count: the buffer is refilled at the new size
    x2 = np.linspace(-5, 5, 333).reshape(-1, 1).astype(np.float32)
    eng.bind_points(torch.as_tensor(x2, device="cuda"))
    v2 = eng.orth_values(0)
    assert tuple(v2.shape) == (333,)
    assert close(v2.cpu().numpy(), _oracle_psi(kw, theta, x2, 0, 0.37), 5e-6, 2e-6)
    eng.step()
    assert _same_bits(eng.orth_values(0), v2)
    # clearing restores the plain step
    eng.bind_points(torch.as_tensor(x, device="cuda"))
    eng.bind_orth_state(0, None)
    _raises(capi.GPE_ERR_STATE, eng.orth_values, 0)
    eng.set_perturb_scale(1.0)
    eng.set_gamma(3.0)
    eng.set_params(flat)
    eng.reset_optimizer(1e-3)
    o0, g0, _ = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64))
    sc0 = eng.step()
    assert sc0["orth"] == 0.0 and abs(sc0["loss"] - o0["loss"]) <= 1e-4 * abs(o0["loss"])
    assert H.rel_err(eng.get_grad(), g0) < 5e-5
    eng.close()


# ---- 5. two halves of a sampled grid ------------------------------------------------------------------------------------------------
def test_two_halves_fill_their_own_rows():
    kw = dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, w_orth=3.0, dx=36.0 / (61 * 47))
    _, flat, x_bc = _inputs(kw, 100)
    n = 61 * 47
    cut = n // 2 + 3                                  # no multiple of the last axis, nor of the 16-point tile
    pb = go.Problem(**kw, n_global=n)
    thetas = [_frozen(kw, 1), _frozen(kw, 2)]
    g = dict(lo=(-3.0, -3.0), hi=(3.0, 3.0), shape=(61, 47), seed=606, every=2)
    full = make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc)
    halves = [make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc, world_size=2) for _ in range(2)]
    for e in [full] + halves:
        for j, th in enumerate(thetas):
            e.bind_orth_state(j, th, amplitude=0.5 + j)
    full.bind_sampler(**g)
    halves[0].bind_sampler(first_cell=0, n=cut, **g)
    halves[1].bind_sampler(first_cell=cut, n=n - cut, **g)
    for step in range(3):                             # the third step runs on a redrawn set
        ref = full.step()
        for e in halves:
            e.step_begin()
        tot = halves[0].exchange_sums + halves[1].exchange_sums
        for e in halves:
            e.exchange_sums.copy_(tot)
            e.step_backward()
        gt = halves[0].exchange_grad + halves[1].exchange_grad
        for e in halves:
            e.exchange_grad.copy_(gt)
            e.step_update()
        for e in halves:
            sc = e.read_scalars()
            assert ref["orth"] > 0 and abs(sc["orth"] - ref["orth"]) <= 1e-5 * ref["orth"], step
            assert abs(sc["loss"] - ref["loss"]) <= 1e-5 * abs(ref["loss"]), step
        assert full.sampler_points()[1] == halves[0].sampler_points()[1] == halves[1].sampler_points()[1] == step // 2
        for j in range(2):
            assert _same_bits(torch.cat([halves[0].orth_values(j), halves[1].orth_values(j)]), full.orth_values(j)), (step, j)
    for e in [full] + halves:
        e.close()


# ---- 6. refusals and lifetime -------------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime():
    kw = dict(layers=[2, 32, 32, 1], gamma=1.0, dx=0.01, w_orth=2.0)
    x, flat, _ = _inputs(kw, 400)
    theta = _frozen(kw)
    g = dict(lo=(-3.0, -3.0), hi=(3.0, 3.0), shape=(20, 20), every=2)
    eng = make_engine(go.Problem(**kw), flat, x)
    _raises(capi.GPE_ERR_STATE, eng.orth_values, 0)                                   # nothing bound
    _raises(capi.GPE_ERR_INVALID, eng.bind_orth_state, 0, theta[:-1])                 # n != param_count
    _raises(capi.GPE_ERR_INVALID, eng.bind_orth_state, -1, theta)
    _raises(capi.GPE_ERR_INVALID, eng.bind_orth_state, capi.GPE_MAX_ORTH, theta)
    _raises(capi.GPE_ERR_INVALID, eng.orth_values, capi.GPE_MAX_ORTH)
    _raises(capi.GPE_ERR_INVALID, eng.bind_orth_state, 0, theta, base_mode=0)         # a base in 2D
    for bad in (float("nan"), float("inf")):
        _raises(capi.GPE_ERR_INVALID, eng.bind_orth_state, 0, theta, perturb_scale=bad)
        _raises(capi.GPE_ERR_INVALID, eng.bind_orth_state, 0, theta, amplitude=bad)
    # a failed bind leaves the previous content of the slot working: a frozen state ...
    eng.bind_orth_state(0, theta, amplitude=0.9)
    v = eng.orth_values(0)
    _raises(capi.GPE_ERR_INVALID, eng.bind_orth_state, 0, theta[:-1])
    _raises(capi.GPE_ERR_INVALID, eng.bind_orth_state, 0, theta, amplitude=float("nan"))
    assert _same_bits(eng.orth_values(0), v)
    assert eng.step()["orth"] > 0
    # ... or a caller array
    arr = torch.full((400,), 0.25, device="cuda")
    eng.bind_orth(0, arr)
    _raises(capi.GPE_ERR_STATE, eng.orth_values, 0)                                   # the array replaced the state
    _raises(capi.GPE_ERR_INVALID, eng.bind_orth_state, 0, theta[:-1])
    assert eng.step()["orth"] > 0
    # the sampler refuses caller arrays, not frozen states; an array under a sampler stays refused
    _raises(capi.GPE_ERR_INVALID, eng.bind_sampler, **g)
    eng.bind_orth_state(0, theta)                                                     # the state replaces the array
    eng.bind_sampler(**g)
    assert eng.step()["orth"] > 0
    _raises(capi.GPE_ERR_STATE, eng.bind_orth, 0, arr)
    assert tuple(eng.orth_values(0).shape) == (400,)                                  # the refused array changed nothing
    eng.bind_orth_state(1, _frozen(kw, 2))                                            # binding under a sampler fills on its set
    pts, _ = eng.sampler_points()
    assert close(eng.orth_values(1).cpu().numpy(), _oracle_psi(kw, _frozen(kw, 2), pts.cpu().numpy()), 5e-6, 2e-6)
    eng.run(5)
    eng.clear_sampler()
    _raises(capi.GPE_ERR_STATE, eng.orth_values, 0)                                   # no points bound
    eng.bind_orth(1, None)                                                            # bind_orth(k, NULL) clears a frozen state too
    eng.bind_points(torch.as_tensor(x, device="cuda"))
    _raises(capi.GPE_ERR_STATE, eng.orth_values, 1)
    assert close(eng.orth_values(0).cpu().numpy(), _oracle_psi(kw, theta, x), 5e-6, 2e-6)
    for i in range(50):                                                               # bind / clear cycles: no error returned
        eng.bind_orth_state(0, theta, amplitude=1.0 + i)
        eng.bind_orth_state(0, None)
    assert eng.step()["orth"] == 0.0
    eng.close()
    # complex psi, and a precomputed base
    cx = gpe_pinn.Engine(gpe_pinn.GPEConfig(layers=[2, 32, 32, 2], complex_psi=True, gamma=1.0, dx=0.01, w_bc=0.0))
    _raises(capi.GPE_ERR_INVALID, cx.bind_orth_state, 0, np.zeros(cx.n_params, np.float32))
    cx.close()
    pre = gpe_pinn.Engine(gpe_pinn.GPEConfig(layers=[1, 32, 32, 1], gamma=1.0, dx=0.01, w_bc=0.0, base_mode=0, base_kind=capi.BASE_PRECOMPUTED))
    z = np.zeros(pre.n_params, np.float32)
    _raises(capi.GPE_ERR_INVALID, pre.bind_orth_state, 0, z, base_mode=1)
    pre.bind_orth_state(0, z)                                                         # without a base it is fine
    pre.close()


def test_another_engine_as_the_frozen_state():
    """Engine.bind_orth_state(k, other_engine) takes the other engine's parameters, base_mode and perturb_scale."""
    kw = dict(layers=[1, 32, 32, 1], gamma=1.0, dx=0.03, base_mode=1, perturb_scale=0.2)
    x, flat, _ = _inputs(kw, 300)
    low = make_engine(go.Problem(**{**kw, "base_mode": 0, "perturb_scale": 0.4}), _frozen(kw), x)
    eng = make_engine(go.Problem(**kw, w_orth=1.0), flat, x)
    eng.bind_orth_state(0, low, amplitude=1.5)
    assert close(eng.orth_values(0).cpu().numpy(), _oracle_psi(kw, _frozen(kw), x, 0, 0.4, 1.5), 5e-6, 2e-6)
    low.close(); eng.close()
