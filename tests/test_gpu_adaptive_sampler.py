"""Residual-adaptive sampler (include/gpe_hip.h: gpe_sampler_adaptive) on the device, held to its numpy restatement
(gpe_pinn.sampler: adaptive_counts / adaptive_points / adaptive_weights), to the engine's own residual, and to a host loop of
bind_points + bind_weights.  One small shape per kernel family plus the two-output cases; every = 4; every set has <= 1 024 rows, so a
weighted step adds its sums in one head workgroup and is bit-reproducible."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import Engine, GPEConfig, GPEError, capi
from gpe_pinn import sampler as S
from oracle import gpe_oracle as go

pytestmark = pytest.mark.gpu

EVERY, SEED, DRAW0, N_MIN, SHARE = 4, 2024, 3, 2, 0.25
COMMON = dict(gamma=20.0, dx=1.0, w_bc=0.0, lr=1e-2)
# name: (config, block edges per axis, N)
CASES = {
    "1d_64x3": (dict(layers=[1, 64, 64, 64, 1]), [S.sinh_edges(6.0, 8, 2.0)], 256),
    "2d_64x2": (dict(layers=[2, 64, 64, 1]), [S.sinh_edges(4.0, 5, 1.5), np.linspace(-3, 3, 5)], 1000),          # no tile multiple
    "2d_128x3_wide": (dict(layers=[2, 128, 128, 128, 1]), [S.sinh_edges(4.0, 3, 1.0), S.sinh_edges(3.0, 3, 2.0)], 600),
    "2d_48x2_generic": (dict(layers=[2, 48, 48, 1], path=gpe_pinn.PATH_GENERIC), [np.linspace(-3, 3, 3), S.sinh_edges(3.0, 3, 1.5)], 300),
    "2d_64x2_complex": (dict(layers=[2, 64, 64, 2], complex_psi=True, omega_rot=0.5), [S.sinh_edges(4.0, 4, 1.5)] * 2, 512),
    "2d_64x3_mixture": (dict(layers=[2, 64, 64, 64, 2], mixture=True, mix_g=(20.0, 15.0, 25.0), mix_norm=(0.6, 0.4), gamma=0.0),
                        [S.sinh_edges(4.0, 4, 1.5)] * 2, 512),
}
ALL = sorted(CASES)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def edges_of(name):
    return [np.asarray(a, np.float32) for a in CASES[name][1]]


def start_params(name, seed=0):
    layers = CASES[name][0]["layers"]
    scale = 0.3 if max(layers[1:-1]) <= 64 else 0.15
    return (np.random.default_rng(77 + seed).normal(0, 1, go.param_count(layers)) * scale).astype(np.float32)


def engine(name, flat=None):
    kw = dict(COMMON)
    kw.update(CASES[name][0])
    eng = Engine(GPEConfig(**kw))
    eng.set_params(start_params(name) if flat is None else flat)
    return eng


def adaptive(name, share=SHARE, flat=None, **kw):
    eng = engine(name, flat)
    args = dict(every=EVERY, seed=SEED, n_min=N_MIN, uniform_share=share, draw0=DRAW0)
    args.update(kw)
    eng.bind_sampler_adaptive(edges_of(name), CASES[name][2], **args)
    return eng


def volume_counts(name):
    return S.adaptive_counts(None, 0.0, edges_of(name), CASES[name][2], N_MIN, S.uniform_per_1024(SHARE))


def full_state(eng):
    return (eng.get_params(),) + tuple(eng.get_adam_state()[:2])


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


# ---- 1. allocation and draw, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_counts_points_and_weights_equal_the_numpy_restatement_after_every_redraw(name):
    """Every case moves points at its first redraw already: the start parameters are random, the trap's V u dominates the residual in
    the outer blocks, and with uniform_share = 0.25 three quarters of the spare rows follow it (seen on the first GPU run: no case
    of the table kept the allocation by volume at any of its three redraws)."""
    ed, N = edges_of(name), CASES[name][2]
    s = S.uniform_per_1024(SHARE)
    eng = adaptive(name)
    st = eng.adaptive_state()
    assert st["draw"] == DRAW0 and st["total"] == 0.0 and not st["mass"].any()          # the bind: by volume, nothing evaluated
    assert np.array_equal(st["counts"], volume_counts(name))
    moved = 0
    for m in range(0, 4):
        if m:
            eng.run(EVERY if m == 1 else EVERY - 1)   # up to step m * every - 1 ...
            eng.step()                                # ... and step m * every: the redraw fires in front of it
        st = eng.adaptive_state()
        counts = st["counts"]
        assert st["draw"] == DRAW0 + m and counts.sum() == N and counts.min() >= N_MIN
        if m:
            assert st["total"] > 0 and np.isfinite(st["total"]) and (st["mass"] >= 0).all()
        assert np.array_equal(counts, S.adaptive_counts(st["mass"], st["total"], ed, N, N_MIN, s)), (name, m)
        pts, draw = eng.sampler_points()
        w = eng.weights()
        assert draw == DRAW0 + m and pts.shape == (N, len(ed))
        assert np.array_equal(bits(pts.cpu().numpy()), bits(S.adaptive_points(ed, counts, SEED, DRAW0 + m))), (name, m)
        assert np.array_equal(bits(w["q"].cpu().numpy()), bits(S.adaptive_weights(ed, counts))), (name, m)
        assert w["total"] == S.graded_total(ed)
        moved += int(m > 0 and not np.array_equal(counts, volume_counts(name)))
        print(f"[adaptive] {name} redraw {m}: counts {counts.tolist()}  M {st['total']:.6g}")
    assert moved >= 1, (name, moved)
    eng.close()


def test_a_clip_box_narrower_than_the_blocks_is_honoured():
    name = "2d_64x2"
    clip = ((-3.5, -2.5), (3.5, 2.5))
    eng = adaptive(name, clip=clip)
    eng.run(EVERY + 1)
    st = eng.adaptive_state()
    pts = eng.sampler_points()[0].cpu().numpy()
    assert np.array_equal(bits(pts), bits(S.adaptive_points(edges_of(name), st["counts"], SEED, DRAW0 + 1, clip=clip)))
    assert pts[:, 0].min() >= -3.5 and pts[:, 0].max() <= 3.5 and pts[:, 1].min() >= -2.5 and pts[:, 1].max() <= 2.5
    eng.close()


# ---- 2. masses against the engine's own residual ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_block_masses_equal_fp64_host_sums_over_the_engines_own_residual(name):
    """Both sides add the same terms double(q_i) * sum_c double(r_ic)^2 (each exact up to one rounding made alike on both sides) in
    fp64, in different orders: two sums of n non-negative terms differ by at most 2 (n - 1) 2^-53 of their value, so
    |m_b - ref_b| <= n_b 2^-52 ref_b and |M - ref| <= N 2^-52 ref."""
    ed, N = edges_of(name), CASES[name][2]
    a = adaptive(name)
    a.run(EVERY)
    counts = a.adaptive_state()["counts"].astype(np.int64)          # the set the masses are about to be formed on
    pts, q = a.sampler_points()[0], a.weights()["q"]
    b = engine(name, a.get_params())
    b.bind_points(pts)
    b.bind_weights(q, total=S.graded_total(ed))
    _, _, res = b.residual()
    b.close()
    term = q.cpu().numpy().astype(np.float64) * (res.cpu().numpy().astype(np.float64) ** 2).sum(axis=1)
    off = np.concatenate([[0], np.cumsum(counts)])
    ref = np.array([term[off[i]:off[i + 1]].sum() for i in range(counts.size)])
    a.step()                                          # fires the redraw, and the detour in front of it
    st = a.adaptive_state()
    a.close()
    assert st["draw"] == DRAW0 + 1 and (ref > 0).all()
    err = np.abs(st["mass"] - ref)
    print(f"[adaptive] {name}: max |m_b - ref| / ref = {(err / ref).max():.3e}, |M - ref| / ref = {abs(st['total'] - ref.sum()) / ref.sum():.3e}")
    assert (err <= counts * 2.0 ** -52 * ref).all(), (name, (err / ref).max())
    assert abs(st["total"] - ref.sum()) <= N * 2.0 ** -52 * ref.sum()


# ---- 3. the detour leaves the trajectory alone ----------------------------------------------------------------------------------------
def host_loop(name, counts_per_draw, chunks):
    ed = edges_of(name)
    b = engine(name)
    for m, (counts, k) in enumerate(zip(counts_per_draw, chunks)):
        b.bind_points(dev(S.adaptive_points(ed, counts, SEED, DRAW0 + m)))
        b.bind_weights(dev(S.adaptive_weights(ed, counts)), total=S.graded_total(ed))
        b.run(k)
    return b


def same_trajectory(a, b, steps):
    for p, r in zip(full_state(a), full_state(b)):
        assert np.array_equal(bits(p), bits(r))
    assert a.get_adam_state()[2] == b.get_adam_state()[2] == steps
    assert np.array_equal(bits(a.read_history_array(1, steps)), bits(b.read_history_array(1, steps)))          # (steps count from 1)


@pytest.mark.parametrize("name", ALL)
def test_adaptive_run_equals_a_host_loop_of_bind_points_and_bind_weights(name):
    steps, chunks = 3 * EVERY + 2, (EVERY, EVERY, EVERY, 2)
    a = adaptive(name)
    counts = []
    for k in chunks:
        a.run(k)
        counts.append(a.adaptive_state()["counts"].copy())          # of the draw this chunk ran on
    assert a.adaptive_state()["draw"] == DRAW0 + 3
    b = host_loop(name, counts, chunks)
    same_trajectory(a, b, steps)
    a.close(); b.close()


@pytest.mark.parametrize("name", ["2d_64x2", "2d_64x2_complex"])
def test_with_every_row_allocated_by_volume_the_masses_are_evaluated_and_ignored(name):
    steps, chunks = 3 * EVERY + 2, (EVERY, EVERY, EVERY, 2)
    with environment({"GPE_GRAPH_STEPS": "4"}):       # (a graph of 4 steps fits between two redraws: the default 8 would never replay)
        a = adaptive(name, share=1.0)
    a.run(steps)                                      # one call: graph replays, cut at the redraws
    st = a.adaptive_state()
    by_volume = S.adaptive_counts(None, 0.0, edges_of(name), CASES[name][2], N_MIN, 1024)
    assert st["draw"] == DRAW0 + 3 and st["total"] > 0 and np.array_equal(st["counts"], by_volume)
    b = host_loop(name, [by_volume] * 4, chunks)
    same_trajectory(a, b, steps)
    a.close(); b.close()


# ---- 4. graph replay ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d_64x2", "2d_64x3_mixture"])
def test_graph_replays_and_plain_launches_agree_bit_for_bit(name):
    """GPE_GRAPH_STEPS = 4: with the default of 8 steps per graph a redraw every 4 steps would leave no room for a single replay"""
    got = {}
    for g in ("1", "0"):
        with environment({"GPE_GRAPH": g, "GPE_GRAPH_STEPS": "4"}):
            eng = adaptive(name)
            eng.run(3 * EVERY + 2)
            got[g] = (full_state(eng), eng.adaptive_state(), eng.sampler_points()[0].cpu().numpy())
            eng.close()
    for p, r in zip(got["1"][0], got["0"][0]):
        assert np.array_equal(bits(p), bits(r))
    s1, s0 = got["1"][1], got["0"][1]
    assert s1["draw"] == s0["draw"] == DRAW0 + 3 and s1["total"] == s0["total"] > 0
    assert np.array_equal(bits(s1["mass"]), bits(s0["mass"])) and np.array_equal(s1["counts"], s0["counts"])
    assert np.array_equal(bits(got["1"][2]), bits(got["0"][2]))


# ---- 5. run to run --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d_128x3_wide", "2d_64x2_complex"])
def test_two_engines_with_the_same_seed_hold_the_same_masses_counts_and_points(name):
    got = []
    for _ in range(2):
        eng = adaptive(name)
        eng.run(2 * EVERY + 1)
        got.append((eng.adaptive_state(), eng.sampler_points()[0].cpu().numpy()))
        eng.close()
    (sa, pa), (sb, pb) = got
    assert sa["draw"] == sb["draw"] == DRAW0 + 2 and sa["total"] == sb["total"] > 0
    assert np.array_equal(bits(sa["mass"]), bits(sb["mass"])) and np.array_equal(sa["counts"], sb["counts"])
    assert np.array_equal(bits(pa), bits(pb))


# ---- 6. a NaN among the parameters ----------------------------------------------------------------------------------------------------
def test_a_nan_parameter_falls_back_to_the_allocation_by_volume():
    name = "2d_64x2"
    flat = start_params(name)
    flat[10] = np.nan
    eng = adaptive(name, flat=flat)
    eng.run(EVERY + 1)
    st = eng.adaptive_state()
    assert st["draw"] == DRAW0 + 1 and not (st["total"] > 0 and np.isfinite(st["total"]))
    assert np.array_equal(st["counts"], volume_counts(name))
    pts = eng.sampler_points()[0].cpu().numpy()
    assert np.array_equal(bits(pts), bits(S.adaptive_points(edges_of(name), st["counts"], SEED, DRAW0 + 1)))
    eng.close()


# ---- 7. refusals and lifetime -----------------------------------------------------------------------------------------------------------
def _code(fn, *a, **k):
    with pytest.raises(GPEError) as ex:
        fn(*a, **k)
    return ex.value.code


def test_refusals_and_lifetime():
    name = "2d_64x2"
    ed, N = edges_of(name), CASES[name][2]
    B = 20
    eng = engine(name)
    assert _code(eng.adaptive_state) == capi.GPE_ERR_STATE                        # nothing bound
    bind = lambda **kw: eng.bind_sampler_adaptive(ed, **{**dict(n_points=N, every=EVERY, seed=SEED, n_min=N_MIN, uniform_share=SHARE), **kw})
    assert _code(bind, n_points=(1 << 22) + 1) == capi.GPE_ERR_INVALID
    assert _code(bind, n_points=B * N_MIN - 1) == capi.GPE_ERR_INVALID            # B * n_min > N
    assert _code(bind, n_min=0) == capi.GPE_ERR_INVALID
    assert _code(bind, every=0) == capi.GPE_ERR_INVALID
    assert _code(bind, clip=((1.0, 1.0), (0.0, 0.0))) == capi.GPE_ERR_INVALID
    # what the Python layer cannot express: uniform_per_1024 outside [1, 1024], a block of cells, bad edges
    sp = capi.gpe_sampler_spec()
    for k in range(2):
        sp.shape[k], sp.lo[k], sp.hi[k] = ed[k].size - 1, float(ed[k][0]), float(ed[k][-1])
        sp.clip_lo[k], sp.clip_hi[k] = sp.lo[k], sp.hi[k]
    sp.n_local, sp.every = B, EVERY
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda s, e0, e1, n=N, nmin=N_MIN, u=256: eng.lib.gpe_sampler_adaptive(eng._h, C.byref(s), e0, e1, None, n, nmin, u)
    assert call(sp, ptr(ed[0]), ptr(ed[1]), u=0) == capi.GPE_ERR_INVALID
    assert call(sp, ptr(ed[0]), ptr(ed[1]), u=1025) == capi.GPE_ERR_INVALID
    sp.first_cell, sp.n_local = 1, B - 1
    assert call(sp, ptr(ed[0]), ptr(ed[1])) == capi.GPE_ERR_INVALID               # single-rank: the whole grid
    sp.first_cell, sp.n_local = 0, B - 1
    assert call(sp, ptr(ed[0]), ptr(ed[1])) == capi.GPE_ERR_INVALID
    sp.n_local = B
    flat_edge = ed[0].copy(); flat_edge[2] = flat_edge[1]
    assert call(sp, ptr(flat_edge), ptr(ed[1])) == capi.GPE_ERR_INVALID
    assert call(sp, ptr(ed[0]), None) == capi.GPE_ERR_INVALID
    assert call(sp, ptr(ed[0]), ptr(ed[1]), u=1) == capi.GPE_OK and call(sp, ptr(ed[0]), ptr(ed[1]), u=1024) == capi.GPE_OK
    st = eng.adaptive_state()                                                     # bound through the raw ABI: the wrapper asks the engine for B
    assert st["counts"].shape == st["mass"].shape == (B,) and st["counts"].sum() == N
    nb, npts = C.c_int64(), C.c_int64()
    assert eng.lib.gpe_sampler_adaptive_blocks(eng._h, C.byref(nb), C.byref(npts)) == 0 and (nb.value, npts.value) == (B, N)
    with pytest.raises(ValueError):
        bind(uniform_share=0.0)
    # lifetime
    bind()
    p0 = C.c_void_p()
    assert eng.lib.gpe_sampler_points(eng._h, C.byref(p0), None, None) == 0
    q = dev(np.ones(N))
    assert _code(eng.bind_weights, q) == capi.GPE_ERR_STATE and _code(eng.clear_weights) == capi.GPE_ERR_STATE
    assert _code(eng.step_dp) == capi.GPE_ERR_STATE and _code(eng.run_dp, 2) == capi.GPE_ERR_STATE
    assert eng.lib.gpe_comm_init(eng._h, b"\0" * 128, 0, 1) == capi.GPE_ERR_STATE
    eng.run(EVERY + 1)
    bind(seed=SEED + 1)                                                           # a rebind with the same N keeps the point buffer
    p1 = C.c_void_p()
    assert eng.lib.gpe_sampler_points(eng._h, C.byref(p1), None, None) == 0 and p1.value == p0.value
    st = eng.adaptive_state()
    assert st["draw"] == 0 and st["total"] == 0.0 and np.array_equal(st["counts"], volume_counts(name))
    assert eng.weights()["total"] == S.graded_total(ed)
    eng.bind_points(dev(np.zeros((50, 2))))                                       # the caller's points take over
    assert _code(eng.adaptive_state) == capi.GPE_ERR_STATE and _code(eng.weights) == capi.GPE_ERR_STATE
    assert _code(eng.sampler_points) == capi.GPE_ERR_STATE
    bind()
    eng.clear_sampler()                                                           # gpe_bind_sampler(NULL) clears it too
    assert _code(eng.adaptive_state) == capi.GPE_ERR_STATE and _code(eng.weights) == capi.GPE_ERR_STATE
    bind()
    eng.bind_sampler_graded(ed, every=EVERY)                                      # ... and a sampler of another kind replaces it
    assert _code(eng.adaptive_state) == capi.GPE_ERR_STATE and eng.weights()["q"].numel() == B
    eng.step()
    eng.close()
    # an engine with a communicator: GPE_ERR_STATE, and the graded sampler it held stays in place and steps on
    dp = engine(name)
    dp.bind_sampler_graded(ed, every=EVERY, seed=SEED)
    dp.comm_init(0, 1)
    assert _code(dp.bind_sampler_adaptive, ed, N, every=EVERY, seed=SEED, n_min=N_MIN, uniform_share=SHARE) == capi.GPE_ERR_STATE
    assert _code(dp.adaptive_state) == capi.GPE_ERR_STATE
    pts, draw = dp.sampler_points()
    assert draw == 0 and np.array_equal(bits(pts.cpu().numpy()), bits(S.graded_points(ed, SEED, 0))) and dp.weights()["q"].numel() == B
    dp.step_dp()
    dp.close()
    sym = Engine(GPEConfig(**{**COMMON, **CASES[name][0], "w_sym": 5.0}))          # the symmetry batch has no weights
    assert _code(sym.bind_sampler_adaptive, ed, N, every=EVERY) == capi.GPE_ERR_INVALID
    sym.close()


# ---- 8. frozen orthogonality states ---------------------------------------------------------------------------------------------------
def test_a_frozen_orthogonality_state_is_refilled_behind_an_adaptive_redraw():
    name = "1d_64x3"
    theta = start_params(name, seed=5)
    kw = {**COMMON, **CASES[name][0], "w_orth": 2.0}
    eng = Engine(GPEConfig(**kw))
    eng.set_params(start_params(name))
    eng.bind_orth_state(0, theta)
    eng.bind_sampler_adaptive(edges_of(name), CASES[name][2], every=EVERY, seed=SEED, n_min=N_MIN, uniform_share=SHARE)
    ref = Engine(GPEConfig(**kw))
    ref.set_params(theta)
    psi0 = eng.orth_values(0).cpu().numpy()
    assert np.array_equal(bits(psi0), bits(ref.forward(eng.sampler_points()[0]).cpu().numpy()[:, 0]))
    eng.run(EVERY + 1)
    pts, draw = eng.sampler_points()
    psi1 = eng.orth_values(0).cpu().numpy()
    assert draw == 1 and not np.array_equal(psi0, psi1)
    assert np.array_equal(bits(psi1), bits(ref.forward(pts).cpu().numpy()[:, 0]))
    eng.close(); ref.close()
