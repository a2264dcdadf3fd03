"""The engine's device-side stratified sampler (include/gpe_hip.h: gpe_bind_sampler, csrc/gpe_sampler.h) against its numpy
restatement gpe_pinn.sampler.stratified_points (bit for bit), its cadence through every step entry point, one training step on a
sampled set against the fp64 oracle, and the identity of a sampled trajectory with the one a host loop of bind_points gives."""
import math

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import capi
from gpe_pinn.sampler import stratified_points
from oracle import gpe_oracle as go
from tests import helpers as H
from tests.test_gpu_parity import CASES, PATHS, _inputs, _scale, close, make_engine

pytestmark = pytest.mark.gpu

LO = (-3.0, -2.5, -2.0)
HI = (3.0, 3.5, 2.25)


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _small_engine(d, **kw):
    cfg = gpe_pinn.GPEConfig(layers=[d, 32, 32, 1], gamma=1.0, dx=0.01, w_bc=0.0, **kw)
    eng = gpe_pinn.Engine(cfg)
    rng = np.random.default_rng(3)
    eng.set_params((rng.normal(0, 1, eng.n_params) * 0.3).astype(np.float32))
    return eng


def _shape_for(d, cells):
    """a grid of d axes with at least `cells` cells whose last axes are no powers of two"""
    if d == 1:
        return (cells + 11,)
    if d == 2:
        return (-(-cells // 301) + 1, 301)
    return (-(-cells // (13 * 11)) + 1, 13, 11)


# ---- 1. the device set is stratified_points, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 17, 4099, 300 * 300])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_device_set_equals_numpy_restatement_bit_for_bit(d, N):
    eng = _small_engine(d)
    for first_cell, clip in ((0, None), (29, None), (7, (tuple(-1.75 + 0.25 * k for k in range(d)), tuple(1.5 + 0.125 * k for k in range(d))))):
        shape = _shape_for(d, first_cell + N)
        for draw0 in (0, 1, 2 ** 33 + 5):
            g = dict(lo=LO[:d], hi=HI[:d], shape=shape, seed=0x1234567887654321 + draw0, first_cell=first_cell, n=N, clip=clip)
            eng.bind_sampler(every=3, draw0=draw0, **g)
            pts, draw = eng.sampler_points()
            assert draw == draw0 and tuple(pts.shape) == (N, d) and pts.dtype == torch.float32
            want = stratified_points(draw=draw0, **g)
            assert np.array_equal(_bits(pts), _bits(want)), (d, N, first_cell, draw0, clip)
            if clip is not None:
                for k in range(d):
                    assert float(pts[:, k].min()) >= np.float32(clip[0][k]) and float(pts[:, k].max()) <= np.float32(clip[1][k])
    eng.close()


# ---- 2. cadence: after every * m + r steps (r >= 1) the buffer holds draw0 + m ----------------------------------------------------
@pytest.mark.parametrize("every", [5, 16])
def test_cadence_through_step_and_run(every):
    kw = CASES["2d_32x3"][0]
    g = dict(lo=(-3.0, -3.0), hi=(3.0, 3.0), shape=(64, 48), seed=99)          # 3072 points: gpe_run replays its 8-step graph
    draw0 = 4
    _, flat, x_bc = _inputs(kw, 100)

    def engine():
        eng = make_engine(go.Problem(**kw), flat, np.zeros((4, 2), np.float32), x_bc)
        eng.bind_sampler(every=every, draw0=draw0, **g)
        return eng

    def check(eng, total):
        pts, draw = eng.sampler_points()
        m = (total - 1) // every if total > 0 else 0
        assert draw == draw0 + m, (total, draw)
        assert np.array_equal(_bits(pts), _bits(stratified_points(draw=draw, **g))), total

    a = engine()
    check(a, 0)
    for s in range(1, 3 * every + 3):
        a.step()
        check(a, s)
    b = engine()
    total = 0
    for chunk in (1, 8, 2 * every, 3, 17, 40, every, 1):
        b.run(chunk)
        total += chunk
        check(b, total)
    hist = b.read_history(1, total)
    assert [int(h["step"]) for h in hist] == list(range(1, total + 1))
    a.close(); b.close()


# ---- 3. one step on a sampled set against the fp64 oracle (bounds of test_step_matches_oracle) ------------------------------------
ORACLE_CASES = [
    ("2d_64x4_g500", "fused"),                  # fused H = 64
    ("2d_64x4_g500", "generic"),                # generic set
    ("3d_64x3_aniso", "generic"),
    ("1d_64x3_refine", "fused"),                # small batch: the cooperative whole-network kernels
    ("2d_64x5_four_maps", "fused"),
    ("2d_128x5_cfg3", "fused"),                 # wide set, H = 128
    ("3d_256x6_cfg5_N300", "fused"),            # wide set, H = 256
    ("2d_64x3_complex_rot", "fused"),           # complex psi in the rotating frame
    ("2d_64x3_complex_rot", "generic"),
    ("1d_residual_64x2blocks", "generic"),      # residual blocks
    ("2d_residual_64x2blocks", "fused"),
    ("1d_32x4_nb_sym", "fused"),                # w_sym != 0: the [x ; -x] batch must follow the redraw
    ("1d_32x4_nb_sym", "generic"),
    ("1d_64x4_m3_p4_odd", "fused"),
    ("2d_N17_ragged", "fused"),                 # 5 boundary rows against 17 points: a boundary batch of its own (all others: merged)
]


@pytest.mark.parametrize("name,path", ORACLE_CASES)
def test_step_after_a_redraw_matches_oracle(name, path):
    kw, N, _ = CASES[name]
    _, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    d = kw["layers"][0]
    side = N + 3 if d == 1 else math.ceil((N + 3) ** (1.0 / d))
    g = dict(lo=(-6.0,) if d == 1 else (-3.0,) * d, hi=(6.0,) if d == 1 else (3.0,) * d, shape=(side,) * d, seed=2718, first_cell=3, n=N)
    every, draw0 = 2, 6
    eng = make_engine(pb, flat, np.zeros((3, d), np.float32), x_bc, path=PATHS[path])
    assert eng.active_path == PATHS[path]
    eng.bind_sampler(every=every, draw0=draw0, **g)
    for _ in range(every):                           # the steps of draw0; the next one starts with a redraw
        eng.step()
    _, draw = eng.sampler_points()
    assert draw == draw0
    eng.set_params(flat)
    eng.reset_optimizer(1e-3)
    sc = eng.step()                                  # redraws, then runs on draw0 + 1
    pts, draw = eng.sampler_points()
    x = stratified_points(draw=draw0 + 1, **g)
    assert draw == draw0 + 1 and np.array_equal(_bits(pts), _bits(x))
    x64 = pts.cpu().numpy().astype(np.float64)
    osc, ograd, ores = go.full_loss_and_grad(pb, flat.astype(np.float64), x64, x_bc.astype(np.float64))
    _, oskip, oplain = go.expand_layers(pb.layers, pb.net_kind)
    ojets, _ = go.mlp_forward(go.unflatten(flat.astype(np.float64), pb.layers, pb.net_kind), x64, pb.activation, skip=oskip, plain_tanh=oplain)
    f = 10.0 if N < 4 else 1.0
    for k, tol in (("mu", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("bc", 1e-4), ("norm", 2e-4), ("sym", 1e-4), ("riesz", 1e-4), ("reg", 1e-4)):
        assert abs(sc[k] - osc[k]) <= f * tol * max(abs(osc[k]), 1e-6), (k, sc[k], osc[k])
    grad = eng.get_grad()
    assert H.rel_err(grad, ograd) < f * 5e-5
    assert abs(sc["grad_norm"] - np.linalg.norm(ograd)) < f * 1e-4 * np.linalg.norm(ograd)
    new, _, _ = go.optimizer_step(go.OptState(lr0=1e-3), flat, ograd, osc["loss"])
    dd = np.abs(eng.get_params() - new)
    assert np.quantile(dd, 0.99) < 2e-5 and dd.max() < 2.1e-3
    # jets and residual of the same parameters on the set the buffer holds now
    eng.set_params(flat)
    jets = eng.forward_jets(pts).cpu().numpy()
    for c in range(jets.shape[0]):
        assert close(jets[c], ojets[c], 1e-5, 2e-6), f"jet channel {c}"
    rs, psi, res = eng.residual()
    assert close(psi.cpu().numpy(), ores["psi"], 5e-6, 2e-6)
    assert close(res.cpu().numpy(), ores["residual"], 2e-5, 1e-5)
    assert abs(rs["loss"] - osc["loss"]) <= f * 1e-4 * abs(osc["loss"])
    eng.close()


# ---- 4. trajectory identity with the host loop ----------------------------------------------------------------------------------
def _state(eng):
    m, v, step = eng.get_adam_state()
    return eng.get_params(), m, v, step


def _same_state(a, b):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.mark.parametrize("side,every", [(64, 5), (64, 16), (192, 5)], ids=["graph_every5", "graph_every16", "above_graph_threshold"])
def test_trajectory_equals_host_loop_of_bind_points(side, every):
    """sampler + run()  ==  bind_points(stratified_points(draw m)) before each chunk of `every` steps  ==  sampler + step() one by one:
    parameters and Adam moments bit for bit (sched = CONST, default kernels, one GPU); the history loss to 1e-10 relative -- the
    reported loss carries one atomically summed fp64 term, whose reassociation N * 2^-53 bounds."""
    kw = dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=36.0 / (side * side))
    _, flat, x_bc = _inputs(kw, 100)
    pb = go.Problem(**kw)
    g = dict(lo=(-3.0, -3.0), hi=(3.0, 3.0), shape=(side, side), seed=31337)
    steps = 3 * every + 2
    a = make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc, sched=capi.SCHED_CONST)
    a.bind_sampler(every=every, **g)
    a.run(steps)
    b = make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc, sched=capi.SCHED_CONST)
    done = 0
    for m in range(4):
        b.bind_points(torch.as_tensor(stratified_points(draw=m, **g), device="cuda"))
        k = min(every, steps - done)
        b.run(k)
        done += k
    assert done == steps
    c = make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc, sched=capi.SCHED_CONST)
    c.bind_sampler(every=every, **g)
    for _ in range(steps):
        c.step()
    sa, sb, sc = _state(a), _state(b), _state(c)
    assert sa[3] == steps
    assert _same_state(sa, sb), "sampler run() differs from the host loop of bind_points"
    assert _same_state(sa, sc), "sampler run() differs from sampler step()"
    la = np.array([h["loss"] for h in a.read_history(1, steps)])
    lb = np.array([h["loss"] for h in b.read_history(1, steps)])
    lc = np.array([h["loss"] for h in c.read_history(1, steps)])
    assert np.all(np.abs(la - lb) <= 1e-10 * np.abs(lb)) and np.all(np.abs(la - lc) <= 1e-10 * np.abs(lc))
    assert len(set(np.round(la, 12))) == steps            # the sets do change: no two steps report the same loss
    a.close(); b.close(); c.close()


# ---- 5. the three-phase entry points and the data-parallel step honour the sampler ---------------------------------------------------
def test_three_phase_and_dp_entry_points_honour_the_sampler():
    """step_begin / step_backward / step_update and step_dp / run_dp (world 1) redraw like step(): the same draws bit for bit.
    10 000 points: between 6 145 and 32 768 the head sums are formed by k_head_pde in step() and in the phases alike (README,
    Reproducibility), so the three-phase engine runs the kernels of step() in the order of step() and its parameters and Adam
    moments are held to step()'s bit for bit.  The data-parallel step passes sums and gradient through an all-reduce of its own
    (world 1); it is held to the 1e-5 * max(1, |theta|) that test_side_stream_and_graph_replay_change_nothing grants two launch
    forms of the same step over a dozen steps."""
    kw = dict(layers=[2, 64, 64, 64, 1], gamma=50.0, dx=0.01)
    _, flat, x_bc = _inputs(kw, 100)
    pb = go.Problem(**kw)
    g = dict(lo=(-3.0, -3.0), hi=(3.0, 3.0), shape=(100, 100), seed=5)
    every, steps = 3, 7
    engs = [make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc) for _ in range(4)]
    for e in engs:
        e.bind_sampler(every=every, draw0=2, **g)
    a, b, c, d = engs
    c.comm_init(0, 1)
    d.comm_init(0, 1)
    for s in range(steps):
        a.step()
        b.step_begin(); b.step_backward(); b.step_update()
        c.step_dp()
    d.run_dp(steps)
    want = stratified_points(draw=2 + (steps - 1) // every, **g)
    ta = a.get_params()
    for e in engs:
        pts, draw = e.sampler_points()
        assert draw == 2 + (steps - 1) // every
        assert np.array_equal(_bits(pts), _bits(want))
        assert np.abs(e.get_params() - ta).max() <= 1e-5 * max(1.0, np.abs(ta).max())
    assert _same_state(_state(a), _state(b)), "the three phases differ from step()"
    assert np.array_equal(_bits(c.get_params()), _bits(d.get_params()))          # run_dp is step_dp in a loop
    for e in engs:
        e.close()


# ---- 6. rank-count invariance ------------------------------------------------------------------------------------------------------
def test_two_halves_hold_the_set_of_one_engine():
    kw = dict(layers=[3, 32, 32, 1], gamma=5.0, dx=0.01, omega=(1.0, 1.4, 2.0))
    _, flat, _ = _inputs(kw, 10)
    pb = go.Problem(**kw)
    g = dict(lo=LO, hi=HI, shape=(9, 13, 11), seed=77)
    n = 9 * 13 * 11
    cut = n // 2 + 3                                  # no multiple of the last axis
    every = 4
    full, lo_half, hi_half = (make_engine(pb, flat, np.zeros((4, 3), np.float32), n_global=n) for _ in range(3))
    full.bind_sampler(every=every, **g)
    lo_half.bind_sampler(every=every, first_cell=0, n=cut, **g)
    hi_half.bind_sampler(every=every, first_cell=cut, n=n - cut, **g)
    for steps in (0, 2 * every, 1):
        for e in (full, lo_half, hi_half):
            if steps:
                e.run(steps)
        pf, df = full.sampler_points()
        pl, dl = lo_half.sampler_points()
        ph, dh = hi_half.sampler_points()
        assert df == dl == dh
        assert np.array_equal(_bits(torch.cat([pl, ph])), _bits(pf))
        assert np.array_equal(_bits(pf), _bits(stratified_points(draw=df, **g)))
    assert df == 2
    for e in (full, lo_half, hi_half):
        e.close()


# ---- 7. monitor and sampler together ------------------------------------------------------------------------------------------------
def test_monitor_and_sampler_together():
    kw = dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=36.0 / 4096)
    _, flat, x_bc = _inputs(kw, 100)
    pb = go.Problem(**kw)
    g = dict(lo=(-3.0, -3.0), hi=(3.0, 3.0), shape=(64, 64), seed=8)
    steps, every, mon_every = 43, 5, 4
    xm = np.stack([m.ravel() for m in np.meshgrid(np.linspace(-3, 3, 30), np.linspace(-3, 3, 30), indexing="ij")], axis=1).astype(np.float32)
    a = make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc)
    b = make_engine(pb, flat, np.zeros((4, 2), np.float32), x_bc)
    a.bind_sampler(every=every, **g)
    b.bind_sampler(every=every, **g)
    b.bind_monitor(torch.as_tensor(xm, device="cuda"), every=mon_every, dv=36.0 / 900)
    a.run(steps)
    b.run(steps)
    assert _same_state(_state(a), _state(b))
    recs = b.read_monitor()
    assert len(recs) == steps // mon_every
    assert all(int(r["n"]) == xm.shape[0] for r in recs)
    assert [int(r["step"]) for r in recs] == [mon_every * (i + 1) for i in range(len(recs))]
    pa, da = a.sampler_points()
    pb_, db = b.sampler_points()
    assert da == db == (steps - 1) // every and np.array_equal(_bits(pa), _bits(pb_))
    a.close(); b.close()


# ---- 8. refusals and lifetime ------------------------------------------------------------------------------------------------------
def _raises(code, fn, *args, **kw):
    with pytest.raises(gpe_pinn.GPEError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, (ei.value.code, str(ei.value))


def test_specs_the_engine_cannot_honour_are_invalid():
    g = dict(lo=(-3.0, -3.0), hi=(3.0, 3.0), shape=(20, 20), every=5)
    x = torch.as_tensor(np.random.default_rng(0).uniform(-3, 3, (400, 2)).astype(np.float32), device="cuda")
    eng = _small_engine(2)
    eng.bind_points(x)
    eng.step()
    bad = [dict(g, every=0), dict(g, every=-3),
           dict(g, hi=(3.0, -3.0)), dict(g, hi=(-3.0, 3.0)),
           dict(g, clip=((0.0, 1.0), (1.0, 0.5))),
           dict(g, first_cell=399, n=2), dict(g, first_cell=-1, n=5), dict(g, n=401),
           dict(g, lo=-3.0, hi=3.0, shape=(400,)), dict(g, lo=-3.0, hi=3.0, shape=(20, 5, 4))]
    for spec in bad:
        _raises(capi.GPE_ERR_INVALID, eng.bind_sampler, **spec)
        with pytest.raises(gpe_pinn.GPEError):
            eng.sampler_points()                     # nothing was bound
        eng.step()                                   # ... and the caller's points still train
    eng.bind_orth(0, torch.ones(400, device="cuda"))
    _raises(capi.GPE_ERR_INVALID, eng.bind_sampler, **g)
    eng.bind_orth(0, None)
    eng.bind_sampler(**g)                            # the same spec, once nothing lives on fixed points
    eng.step()
    eng.close()
    pre = _small_engine(2, potential=capi.POT_PRECOMPUTED)
    _raises(capi.GPE_ERR_INVALID, pre.bind_sampler, **g)
    pre.bind_points(x, V=torch.zeros(400, device="cuda"))
    _raises(capi.GPE_ERR_INVALID, pre.bind_sampler, **g)
    pre.step()
    pre.close()
    base = gpe_pinn.Engine(gpe_pinn.GPEConfig(layers=[1, 32, 32, 1], gamma=1.0, dx=0.01, w_bc=0.0, base_mode=0, base_kind=capi.BASE_PRECOMPUTED))
    _raises(capi.GPE_ERR_INVALID, base.bind_sampler, lo=-3.0, hi=3.0, shape=(100,), every=5)
    base.close()


def test_arrays_on_fixed_points_are_refused_while_a_sampler_is_bound_and_lifetime():
    g = dict(lo=(-3.0, -3.0), hi=(3.0, 3.0), shape=(20, 20), every=2)
    eng = _small_engine(2)
    _raises(capi.GPE_ERR_STATE, eng.sampler_points)
    eng.bind_sampler(**g)
    ones = torch.ones(400, device="cuda")
    _raises(capi.GPE_ERR_STATE, eng.bind_orth, 0, ones)
    eng.bind_orth(0, None)                           # clearing is no array
    _raises(capi.GPE_ERR_STATE, eng.bind_target, ones)
    _raises(capi.GPE_ERR_STATE, eng.mse_step)
    _raises(capi.GPE_ERR_STATE, eng.mse_loss_grad)
    for _ in range(3):
        eng.step()
    assert eng.sampler_points()[1] == 1              # still usable, still drawing
    # bind_points: the caller's points take over
    x = torch.as_tensor(np.random.default_rng(1).uniform(-3, 3, (300, 2)).astype(np.float32), device="cuda")
    eng.bind_points(x)
    _raises(capi.GPE_ERR_STATE, eng.sampler_points)
    before = x.clone()
    eng.run(5)
    eng.synchronize()
    assert torch.equal(x, before)
    eng.bind_target(torch.ones(300, device="cuda"))  # fixed points again: allowed
    eng.mse_step()
    # clear_sampler leaves nothing bound
    eng.bind_sampler(**g)
    eng.step()
    eng.clear_sampler()
    _raises(capi.GPE_ERR_STATE, eng.step)
    _raises(capi.GPE_ERR_STATE, eng.sampler_points)
    eng.clear_sampler()                              # twice is fine
    eng.bind_sampler(**g)
    eng.step()
    eng.close()
