"""Device-side observables (gpe_observables) and the held-out monitor (gpe_bind_monitor / gpe_read_monitor) on the GPU.

Reference: tests/test_observables_cpu.py:observables_ref applied to the fp64 oracle's jets (pinned against closed forms on the CPU).
Bounds, as tests/test_gpu_parity.py::test_step_matches_oracle holds the same kind of quantity: relative 1e-4 for the parts (norm, kin,
pot, inter, rot, moments, peak density), 2e-5 for mu, mu_lap, energy, times 10 for N < 4.  Sums that cancel (lz, rot, mean_x, var_x) are
held relative to dv * sum |summand|.  res_rms: the residual field's bound there (2e-5 max |r| + 1e-5 per point) carried through the root
mean square: | ||a|| - ||b|| | <= ||a - b|| <= sqrt(dv N) (2e-5 max |r| + 1e-5).
"""
import math

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import Engine
from oracle import gpe_oracle as go
from tests.test_gpu_parity import CASES, PATHS, _inputs, _scale, make_engine
from tests.test_observables_cpu import observables_ref

pytestmark = pytest.mark.gpu

# 1D box base + hard boundary factor: not in the parity table (refine/box_pinn_simulation.py:99-130)
EXTRA = {
    "1d_box_base_env": (dict(layers=[1, 32, 32, 32, 1], kinetic_coeff=1.0, potential=go.POT_NONE, gamma=3.0, base_mode=1,
                             base_kind=go.BASE_BOX, box_L=12.0, envelope=go.ENV_SIN, env_L=12.0, perturb_scale=0.5, dx=12 / 399), 400, True),
}
ALL = {**CASES, **EXTRA}
ORACLE_CASES = ["1d_64x3_refine", "1d_box_base_env", "1d_64x4_m3_p4_odd", "1d_abs_power_p2", "1d_gaussian_pot", "1d_periodic_pot",
                "2d_64x4_g500", "3d_64x3_aniso", "2d_64x3_complex_rot", "2d_complex_rot_variational", "2d_128x3_cfg3like", "2d_256x3",
                "2d_100x2_odd_width", "1d_residual_64x2blocks", "2d_residual_64x2blocks", "2d_N1", "2d_N17_ragged"]
PARTS = ("norm", "kin", "pot", "inter", "peak_density")
TIGHT = ("mu", "mu_lap", "energy")


def _params(names):
    out = []
    for name in names:
        out.append(pytest.param(name, "generic", id=f"{name}-generic"))
        if ALL[name][2]:
            out.append(pytest.param(name, "fused", id=f"{name}-fused"))
    return out


def oracle_jets(pb, flat, x64, chunk=32768):
    _, skip, plain = go.expand_layers(pb.layers, pb.net_kind)
    params = go.unflatten(flat.astype(np.float64), pb.layers, pb.net_kind)
    return np.concatenate([go.mlp_forward(params, x64[i:i + chunk], pb.activation, skip=skip, plain_tanh=plain)[0]
                           for i in range(0, x64.shape[0], chunk)], axis=1)


def check_against(got, ref, scale, N, dv, report=None):
    """every field of the struct against the reference, each printed before it is asserted"""
    f = 10.0 if N < 4 else 1.0
    rows = []

    def hold(key, a, b, bound):
        rows.append((key, a, b, abs(a - b), bound))
        print(f"   {key:14s} got {a:+.12e} ref {b:+.12e} |err| {abs(a - b):.3e} bound {bound:.3e}")

    assert got["n"] == N and abs(got["dv"] - dv) <= 1e-7 * dv
    for k in PARTS:
        hold(k, got[k], ref[k], f * 1e-4 * max(abs(ref[k]), 1e-6))
    for k in TIGHT:
        hold(k, got[k], ref[k], f * 2e-5 * max(abs(ref[k]), 1e-6))
    for k in ("lz", "rot"):
        hold(k, got[k], ref[k], f * 1e-4 * max(scale[k], 1e-6))
    for k in ("mean_x", "var_x"):
        for j in range(3):
            hold(f"{k}[{j}]", got[k][j], ref[k][j], f * 1e-4 * max(scale[k][j], 1e-6))
    hold("res_rms", got["res_rms"], ref["res_rms"], f * math.sqrt(dv * N) * (2e-5 * scale["res_field_max"] + 1e-5))
    if report is not None:
        report.extend(rows)
    bad = [r for r in rows if not r[3] <= r[4]]
    assert not bad, bad


@pytest.mark.parametrize("name,path", _params(ORACLE_CASES))
def test_observables_match_the_fp64_oracle(name, path):
    kw, N, _ = ALL[name]
    x, flat, _ = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    x64 = x.astype(np.float64)
    ref, scale = observables_ref(pb, x64, go.head_pde(pb, x64, oracle_jets(pb, flat, x64)), pb.dx)
    eng = make_engine(pb, flat, x, None, path=PATHS[path])
    assert eng.active_path == PATHS[path]
    got = eng.observables(torch.as_tensor(x, device="cuda"))
    assert got["step"] == 0.0
    check_against(got, ref, scale, N, pb.dx)
    eng.close()


BASELESS = ["2d_64x4_g500", "3d_64x3_aniso", "2d_64x3_complex_rot", "2d_128x3_cfg3like", "2d_N17_ragged", "1d_32x4_cfg1_g0_N2048",
            "3d_256x6_cfg5_N4099"]


@pytest.mark.parametrize("name", BASELESS)
def test_observables_equal_fp64_host_sums_over_the_engines_own_jets(name):
    """norm, kin, inter, lz, moments, peak density against fp64 host sums over forward_jets: the same fp64 products of the same fp32
    numbers, only the order of addition differs (N 2^-53 = 1.2e-10 at 2^20 points; the bound 1e-9 leaves a factor 8 for the rounding of
    the products): a wrong lane, a dropped ragged tail or a double-counted row would show.  Every field is held to 1e-9 relative to
    dv * sum |summand| (normalised like the field); quotients of two such sums included."""
    kw, N, _ = ALL[name]
    assert kw.get("base_mode", -1) < 0 and kw.get("perturb_scale", 1.0) == 1.0
    x, flat, _ = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    eng = make_engine(pb, flat, x, None)
    xd = torch.as_tensor(x, device="cuda")
    J = eng.forward_jets(xd).cpu().numpy().astype(np.float64)
    got = eng.observables(xd)
    eng.close()
    d = x.shape[1]
    x64 = x.astype(np.float64)
    u = J[0]
    rho = (u * u).sum(axis=1)
    sr = rho.sum()
    dv = float(np.float32(pb.dx))                 # the ABI takes the quadrature weight as a float
    I = dv * sr
    p = 3 if pb.complex_psi else pb.p
    g32 = float(np.float32(pb.gamma))
    tol = 1e-9
    assert abs(got["norm"] - I) <= tol * I
    kin = float(np.float32(pb.kinetic_coeff)) * (J[1:1 + d] ** 2).sum() / sr
    assert abs(got["kin"] - kin) <= tol * kin
    s = g32 * rho * rho if pb.complex_psi else g32 * u[:, 0] ** (p + 1)
    inter = 2.0 / (p + 1) * dv * s.sum() / I ** (0.5 * (p + 1))
    assert abs(got["inter"] - inter) <= tol * (2.0 / (p + 1) * dv * np.abs(s).sum() / I ** (0.5 * (p + 1)))
    if pb.complex_psi:
        lz_s = u[:, 0] * (x64[:, 0] * J[2, :, 1] - x64[:, 1] * J[1, :, 1]) - u[:, 1] * (x64[:, 0] * J[2, :, 0] - x64[:, 1] * J[1, :, 0])
        assert abs(got["lz"] - lz_s.sum() / sr) <= tol * np.abs(lz_s).sum() / sr
    else:
        assert got["lz"] == 0.0 and got["rot"] == 0.0
    for k in range(3):
        if k >= d:
            assert got["mean_x"][k] == 0.0 and got["var_x"][k] == 0.0
            continue
        m1, m2, a1 = (x64[:, k] * rho).sum() / sr, (x64[:, k] ** 2 * rho).sum() / sr, (np.abs(x64[:, k]) * rho).sum() / sr
        assert abs(got["mean_x"][k] - m1) <= tol * a1
        assert abs(got["var_x"][k] - (m2 - m1 * m1)) <= tol * (m2 + 2 * abs(m1) * a1)
    assert abs(got["peak_density"] - rho.max() / I) <= tol * rho.max() / I


def test_large_ragged_batch_against_the_oracle():
    """300 001 points of [2,64x4,1]: more points than one sweep of the reduction grid (1024 workgroups of 256), ragged last tile."""
    kw = dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=36.0 / 300001)
    N = 300001
    x, flat, _ = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    x64 = x.astype(np.float64)
    ref, scale = observables_ref(pb, x64, go.head_pde(pb, x64, oracle_jets(pb, flat, x64)), pb.dx)
    eng = make_engine(pb, flat, x, None)
    got = eng.observables(torch.as_tensor(x, device="cuda"))
    eng.close()
    check_against(got, ref, scale, N, pb.dx)


def _bytes(d):
    return np.array([v for k in d for v in (d[k] if isinstance(d[k], list) else [d[k]])], np.float64).tobytes()


def test_records_repeat_bit_for_bit():
    kw, N, _ = CASES["2d_64x3_complex_rot"]
    N = 4099
    x, flat, _ = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw)
    xd = torch.as_tensor(x, device="cuda")
    a = make_engine(pb, flat, x, None)
    b = make_engine(pb, flat, x, None)
    oa1, oa2, ob = a.observables(xd), a.observables(xd), b.observables(xd)
    assert _bytes(oa1) == _bytes(oa2) == _bytes(ob)
    a.close(); b.close()


def test_null_points_mean_the_bound_ones_and_a_precomputed_base_stays_on_them():
    kw = dict(layers=[1, 64, 64, 64, 1], activation=1, kinetic_coeff=1.0, pot_scale=1.0, gamma=3.0, base_mode=2, perturb_scale=0.05, dx=12 / 499)
    x, flat, _ = _inputs(kw, 500)
    a = make_engine(go.Problem(**kw), flat, x, None)
    xd = torch.as_tensor(x, device="cuda")
    oa = a.observables()
    assert _bytes(oa) == _bytes(a.observables(xd))
    phi, p1, p2 = go.hermite_base(x[:, 0].astype(np.float64), 2)
    b = make_engine(go.Problem(**{**kw, "base_kind": go.BASE_PRECOMPUTED}), flat, x, None)
    b.bind_base(phi, p1, p2)
    ob = b.observables()
    for k in ("norm", "energy", "mu", "mu_lap", "res_rms"):          # the same base as three fp32 arrays
        assert abs(ob[k] - oa[k]) <= 1e-5 * abs(oa[k]), k
    with pytest.raises(gpe_pinn.GPEError) as ei:
        b.observables(torch.as_tensor(x[:100] + 0.01, device="cuda"))
    assert ei.value.code == gpe_pinn.capi.GPE_ERR_INVALID and "precomputed base" in str(ei.value)
    with pytest.raises(gpe_pinn.GPEError) as ei:
        b.bind_monitor(torch.as_tensor(x[:100] + 0.01, device="cuda"), every=5)
    assert ei.value.code == gpe_pinn.capi.GPE_ERR_INVALID
    a.close(); b.close()


MON_KW = dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=0.01, lr=1e-3)


def _mon_engine(x, flat, x_bc, env=None):
    import os
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _mon_engine_default(x, flat, x_bc)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _mon_engine_default(x, flat, x_bc):
    return make_engine(go.Problem(**{k: v for k, v in MON_KW.items() if k != "lr"}), flat, x, x_bc, lr=MON_KW["lr"], sched=gpe_pinn.SCHED_CONST)


@pytest.mark.parametrize("N,env", [(4096, {"GPE_GRAPH": "1"}), (20000, {"GPE_GRAPH": "0"})], ids=["graph_replay", "plain_launches"])
def test_monitor_records_equal_stop_and_look(N, env):
    """Engine A: monitor every K = 20 steps on held-out points, run(50) (neither a multiple of K nor of the 8 steps of a replayed graph; at
    4 096 points gpe_run replays graphs and cuts them at the monitor steps, at 20 000 it launches plainly).  Engine B, same start, no
    monitor: run(20), observables(xm), twice.  A's records carry step 20, 40 and equal B's structs byte for byte; A's parameters after 50
    steps equal those of engine C that ran 50 steps with no monitor, byte for byte: the monitor does not disturb training.
    Engine A is created under GPE_GRAPH=1 / GPE_GRAPH=0 (the switch is read at gpe_create), so the two cases do not lean on the default
    (replay up to 16 384 points); B and C run with the defaults.  A (graph, graph, 4 plain steps per 20) and C (6 graphs, 2 plain steps)
    mix replayed and plain steps differently, so their equality also needs a replayed step to equal a plain one bit for bit: the parent
    commit holds that for this shape (tests/switch_table.py: GPE_GRAPH "bitwise", run by tests/test_gpu_switch_matrix.py), so the
    byte-for-byte bound stands and no tolerance is used."""
    K, n = 20, 50
    x, flat, x_bc = _inputs(MON_KW, N)
    xm = np.random.default_rng(5).uniform(-3, 3, (3001, 2)).astype(np.float32)
    xmd = torch.as_tensor(xm, device="cuda")
    a = _mon_engine(x, flat, x_bc, env)
    a.bind_monitor(xmd, every=K, dv=36.0 / 3001)
    a.run(n)
    recs = a.read_monitor()
    assert a.monitor_available() == n // K == len(recs)
    assert [r["step"] for r in recs] == [float(K * (i + 1)) for i in range(n // K)]
    pa = a.get_params()
    a.close()
    b = _mon_engine(x, flat, x_bc)
    for r in recs:
        b.run(K)
        ob = b.observables(xmd, dv=36.0 / 3001)
        assert _bytes(ob) == _bytes(r), (ob, r)
    b.close()
    c = _mon_engine(x, flat, x_bc)
    c.run(n)
    pc = c.get_params()
    c.close()
    np.testing.assert_array_equal(pa, pc)


def test_monitor_ring_keeps_the_newest_and_a_rebind_restarts():
    x, flat, x_bc = _inputs(MON_KW, 1000)
    xmd = torch.as_tensor(np.random.default_rng(6).uniform(-3, 3, (500, 2)).astype(np.float32), device="cuda")
    a = _mon_engine(x, flat, x_bc)
    a.bind_monitor(xmd, every=2, dv=0.07, capacity=3)
    a.run(11)                                                       # records at steps 2, 4, 6, 8, 10
    assert a.monitor_available() == 5
    recs = a.read_monitor()
    assert [r["step"] for r in recs] == [6.0, 8.0, 10.0]
    assert [r["step"] for r in a.read_monitor(3, 2)] == [8.0, 10.0]
    arr = a.read_monitor_array()
    assert arr.shape == (3, len(Engine.OBSERVABLE_FIELDS)) and arr[-1, Engine.OBSERVABLE_FIELDS.index("step")] == 10.0
    with pytest.raises(gpe_pinn.GPEError):
        a.read_monitor(0, 1)                                        # overwritten
    with pytest.raises(gpe_pinn.GPEError):
        a.read_monitor(4, 2)                                        # not written yet
    import ctypes                                                   # a bind the library refuses leaves the monitor and its records
    assert a.lib.gpe_bind_monitor(a._h, ctypes.c_void_p(xmd.data_ptr()), -1, None, 0.07, 2, 3) == gpe_pinn.capi.GPE_ERR_INVALID
    assert a.monitor_available() == 5
    a.clear_monitor()
    a.run(4)
    assert a.monitor_available() == 0 and a.read_monitor() == []
    a.bind_monitor(xmd, every=3, dv=0.07, capacity=3)
    a.run(3)
    recs = a.read_monitor()
    assert len(recs) == 1 and recs[0]["step"] == 18.0               # record 0 again; the optimiser step goes on counting
    a.close()


def test_monitor_on_a_finer_grid_during_a_short_variational_run():
    """The use the monitor exists for, as a test of the wiring (no physics claim about the gap between the grids): train on a coarse 2D
    grid with the variational energy term, monitor a finer grid every K steps."""
    K, n = 25, 300
    ax = np.linspace(-4, 4, 48, dtype=np.float32)
    x = np.stack([m.ravel() for m in np.meshgrid(ax, ax, indexing="ij")], axis=1)
    af = np.linspace(-4, 4, 96, dtype=np.float32)
    xm = np.stack([m.ravel() for m in np.meshgrid(af, af, indexing="ij")], axis=1)
    dv, dvm = float(ax[1] - ax[0]) ** 2, float(af[1] - af[0]) ** 2
    kw = dict(layers=[2, 64, 64, 64, 1], gamma=10.0, dx=dv, w_riesz=1.0, riesz_kind=go.RIESZ_VARIATIONAL)
    _, flat, _ = _inputs(kw, 1)
    eng = make_engine(go.Problem(**kw), flat, x, None, lr=1e-3, sched=gpe_pinn.SCHED_CONST)
    xmd = torch.as_tensor(xm, device="cuda")
    eng.bind_monitor(xmd, every=K, dv=dvm)
    eng.run(n)
    recs = eng.read_monitor()
    assert [r["step"] for r in recs] == [float(K * (i + 1)) for i in range(n // K)]
    for r in recs:
        assert all(np.isfinite(v) for k in r for v in (r[k] if isinstance(r[k], list) else [r[k]])) and r["norm"] > 0
    assert _bytes(recs[-1]) == _bytes(eng.observables(xmd, dv=dvm))
    # two code paths, one definition: the step's own riesz scalar is the energy of the state BEFORE that step's update
    eng.clear_monitor()
    e_before = eng.observables()["energy"]
    sc = eng.step()
    print(f"   energy {e_before:.12e} riesz {sc['riesz']:.12e}")
    assert abs(e_before - sc["riesz"]) <= 2e-5 * abs(sc["riesz"])
    eng.close()


def test_class_surface_observables():
    m = gpe_pinn.pinn2d.GrossPitaevskiiPINN([2, 32, 32, 1], g=10.0)
    ax = np.linspace(0, np.pi, 40, dtype=np.float32)
    X = torch.as_tensor(np.stack([a.ravel() for a in np.meshgrid(ax, ax, indexing="ij")], axis=1), device="cuda")
    o = m.observables(X, float(ax[1] - ax[0]) ** 2)          # (this flavour hands its Gaussian potential over as an array)
    assert o["n"] == 1600 and o["norm"] > 0 and np.isfinite(o["energy"]) and abs(o["energy"] - (o["kin"] + o["pot"] + o["inter"] + o["rot"])) < 1e-12
    m.close()
    r = gpe_pinn.refine.GrossPitaevskiiPINN([1, 32, 32, 1], mode=0, gamma=1.0)       # Hermite base + perturbation, V = x^2, c = 1
    xs = torch.linspace(-8, 8, 801, device="cuda").reshape(-1, 1)
    o = r.observables(xs, 16.0 / 800)
    assert o["n"] == 801 and o["norm"] > 0 and np.isfinite(o["mu"]) and o["var_x"][0] > 0 and o["lz"] == 0.0
    r.close()
