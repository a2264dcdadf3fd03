"""Mixture observables, held-out monitor and keeper on the GPU (include/gpe_hip.h: gpe_mixture_observables, gpe_mixture_monitor,
gpe_mixture_keeper; csrc/gpe_observe_mix.h).

Reference of the oracle cells: tests/mixture_observe_ref.py on the fp64 oracle's jets, pinned on the CPU by
tests/test_mixture_observe_reference_cpu.py (which also shows that every cell can fail).  Bounds, those of tests/test_gpu_observables.py:
relative 1e-4 for the parts (norm, kin, pot, inter, peak density) and the overlap, 2e-5 for mu, mu_lap, energy; sums that cancel
(mean_x, var_x) relative to sum |summand|; res_rms[a] to sqrt(dv N) (2e-5 max |r_a| + 1e-5), res_rms_total to the sum of both bounds.
Own jets and weights: fp64 host sums of the same fp32 numbers, only the order of addition differs: 1e-9.
Monitor and keeper: always against a second engine driven from the host, byte for byte (one GPU repeats a mixture trajectory of one
head workgroup bit for bit: tests/test_gpu_mixture.py::test_run_with_graph_replay_equals_repeated_steps_bit_for_bit)."""
import functools
import math

import numpy as np
import pytest

import gpe_pinn
from gpe_pinn import Engine, GPEConfig, GPEError, capi, keeper
from oracle import gpe_oracle as go
from tests import mixture_cases as mc
from tests import mixture_observe_ref as mo
from tests.test_gpu_mixture import config, dev, make_engine
from tests.test_mixture_observe_reference_cpu import CELLS, cell

pytestmark = pytest.mark.gpu

PARTS = ("norm", "kin", "pot", "inter", "peak_density")
F = Engine.MIXTURE_OBSERVABLE_FIELDS


def _flat(d):
    return np.array([v for k in d for v in np.ravel(d[k])], np.float64)


def _bytes(d):
    return _flat(d).tobytes()


def _raises(code, fn, *args, **kw):
    with pytest.raises(GPEError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, (ei.value.code, str(ei.value))


def hold(rows):
    for key, a, b, bound in rows:
        print(f"   {key:18s} got {a:+.12e} ref {b:+.12e} |err| {abs(a - b):.3e} bound {bound:.3e}")
    bad = [r for r in rows if not abs(r[1] - r[2]) <= r[3]]
    assert not bad, bad


# ---- 1. oracle cells: one per forward family ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CELLS)
def test_matches_the_fp64_reference_on_oracle_jets(name):
    mp, x, flat, _, _, ref, scale = cell(name)
    path = mc.CASES[name][2]
    N, dv = x.shape[0], mp.pb.dx
    eng = make_engine(mp, flat, x, path=path)
    try:
        assert eng.active_path == {"fused": gpe_pinn.PATH_FUSED, "generic": gpe_pinn.PATH_GENERIC}[path]
        got = eng.mixture_observables(dev(x))
    finally:
        eng.close()
    assert got["n"] == N and got["step"] == 0.0 and abs(got["dv"] - dv) <= 1e-7 * dv
    rows = []
    for k in PARTS:
        rows += [(f"{k}[{i}]", got[k][i], ref[k][i], 1e-4 * max(abs(ref[k][i]), 1e-6)) for i in range(len(ref[k]))]
    rows.append(("overlap", got["overlap"], ref["overlap"], 1e-4 * abs(ref["overlap"])))
    for k in ("mu", "mu_lap"):
        rows += [(f"{k}[{a}]", got[k][a], ref[k][a], 2e-5 * max(abs(ref[k][a]), 1e-6)) for a in range(2)]
    rows.append(("energy", got["energy"], ref["energy"], 2e-5 * abs(ref["energy"])))
    for k in ("mean_x", "var_x"):
        rows += [(f"{k}[{a}][{j}]", got[k][a][j], ref[k][a][j], 1e-4 * max(scale[k][a][j], 1e-6)) for a in range(2) for j in range(3)]
    rb = [math.sqrt(dv * N) * (2e-5 * scale["res_field_max"][a] + 1e-5) for a in range(2)]
    rows += [(f"res_rms[{a}]", got["res_rms"][a], ref["res_rms"][a], rb[a]) for a in range(2)]
    rows.append(("res_rms_total", got["res_rms_total"], ref["res_rms_total"], rb[0] + rb[1]))
    hold(rows)
    assert got["energy"] == sum(got["kin"] + got["pot"] + got["inter"])            # the seven fields, added in the struct's order
    lhs, rhs = sum(float(np.float32(mp.n[a])) * got["mu"][a] for a in range(2)), got["energy"] + sum(got["inter"])
    assert abs(lhs - rhs) <= 1e-12 * abs(rhs)


# ---- 2. own jets: only the order of addition differs ------------------------------------------------------------------------------------
OWN_LAYERS = [2, 32, 32, 32, 2]


def _own_engine(N, seed=0):
    """a mixture engine with a PRECOMPUTED potential (so the host sums take the very fp32 numbers the kernel reads), nothing bound"""
    x, flat, _, _ = mc.inputs(OWN_LAYERS, N, seed=seed)
    V = np.random.default_rng(seed + 1).uniform(0.0, 3.0, N).astype(np.float32)
    mp = mc.problem(OWN_LAYERS, N, potential=capi.POT_PRECOMPUTED)
    eng = Engine(config(mp))
    eng.set_params(flat)
    return eng, mp, x, V


def _host_record(eng, mp, x, V, dv, q=None):
    J = eng.forward_jets(dev(x)).cpu().numpy().astype(np.float64)
    f32 = lambda v: [float(np.float32(t)) for t in v]
    return mo.record(J, x.astype(np.float64), V.astype(np.float64), float(np.float32(mp.pb.kinetic_coeff)), f32(mp.g), f32(mp.n),
                     float(np.float32(dv)), q=q)


def _hold_to_host_sums(got, ref, scale, tol=1e-9, dim=2):
    rows = []
    for k in PARTS + ("mu", "res_rms"):
        rows += [(f"{k}[{i}]", got[k][i], ref[k][i], tol * abs(ref[k][i])) for i in range(len(ref[k]))]
    for k in ("energy", "overlap", "res_rms_total"):
        rows.append((k, got[k], ref[k], tol * abs(ref[k])))
    rows += [(f"mu_lap[{a}]", got["mu_lap"][a], ref["mu_lap"][a], tol * (scale["mu_lap"][a] + abs(ref["mu"][a]))) for a in range(2)]
    for k in ("mean_x", "var_x"):
        rows += [(f"{k}[{a}][{j}]", got[k][a][j], ref[k][a][j], tol * scale[k][a][j]) for a in range(2) for j in range(3)]
    hold(rows)
    assert all(got[k][a][j] == 0.0 for k in ("mean_x", "var_x") for a in range(2) for j in range(dim, 3))         # the unused axes


@pytest.mark.parametrize("N", [1, 37, 257, 1025, 262149])
def test_equals_fp64_host_sums_over_the_engines_own_jets(N):
    """257: two slab rows, the second with one live thread; 262 149 = OBS_MAX_WG * 256 + 5: the grid-stride loop wraps"""
    eng, mp, x, V = _own_engine(N)
    dv = 16.0 / N
    try:
        ref, scale = _host_record(eng, mp, x, V, dv)
        got = eng.mixture_observables(dev(x), V=dev(V), dv=dv)
    finally:
        eng.close()
    assert got["n"] == N
    _hold_to_host_sums(got, ref, scale)


# ---- 3. weights on the bound set -----------------------------------------------------------------------------------------------------
def test_integer_weights_equal_the_set_with_repeated_points():
    name = "fused_2d_64x3_N1025"
    mp, x, flat, _, _, _ = mc.case(name)
    q = np.random.default_rng(12).integers(1, 4, x.shape[0]).astype(np.float32)
    idx = np.repeat(np.arange(x.shape[0]), q.astype(np.int64))
    a = make_engine(mp, flat, x, path="fused", q=q)
    b = make_engine(mp, flat, x[idx], path="fused")
    try:
        J, x64 = a.forward_jets(dev(x)).cpu().numpy().astype(np.float64), x.astype(np.float64)
        _, scale = mo.record(J, x64, 0.5 * (x64 ** 2).sum(axis=1), 0.5, mp.g, mp.n, 0.01, q=q)      # sum |summand| of the weighted set
        oa, ob = a.mixture_observables(dv=0.01), b.mixture_observables(dv=0.01)
        plain = a.mixture_observables(dev(x), dv=0.01)                 # an explicit set stays unweighted, even the bound one
    finally:
        a.close(); b.close()
    assert oa["n"] == x.shape[0] and ob["n"] == q.sum()
    _hold_to_host_sums(oa, ob, scale)
    assert abs(plain["norm"][0] - oa["norm"][0]) > 1e-2 * oa["norm"][0]
    # the plain maximum: max u_a^2 is the same number in both, so peak_density = n_a max u_a^2 / I_a differs through the last bits of I_a alone
    for c in range(2):
        assert abs(oa["peak_density"][c] * oa["norm"][c] - ob["peak_density"][c] * ob["norm"][c]) <= 4e-16 * ob["peak_density"][c] * ob["norm"][c]


# ---- 4. repeatability, non-finite state -------------------------------------------------------------------------------------------------
def test_records_repeat_bit_for_bit():
    mp, x, flat, _, _, _ = mc.case("fused_2d_64x3_N1025")
    xs = np.random.default_rng(8).uniform(-2, 2, (4099, 2)).astype(np.float32)
    a, b = make_engine(mp, flat, x), make_engine(mp, flat, x)
    try:
        r1, r2, r3 = a.mixture_observables(dev(xs)), a.mixture_observables(dev(xs)), b.mixture_observables(dev(xs))
        assert _bytes(r1) == _bytes(r2) == _bytes(r3)
        assert _bytes(a.mixture_observables()) == _bytes(a.mixture_observables(dev(x)))      # NULL: the bound points
    finally:
        a.close(); b.close()


def test_nan_parameters_give_a_nan_norm_and_the_keeper_keeps_nothing():
    mp, x, flat, _, _, _ = mc.case("fused_2d_64x3_N37")
    eng = make_engine(mp, np.full_like(flat, np.nan), x)
    try:
        got = eng.mixture_observables(dev(x))
        assert all(np.isnan(v) for v in got["norm"]) and np.isnan(got["energy"]) and np.isnan(got["res_rms_total"])
        assert all(np.isnan(v) for v in got["peak_density"])
        eng.bind_mixture_monitor(dev(x), every=1)
        eng.bind_mixture_keeper("energy", patience=2)
        eng.run(3)
        st = eng.keeper_state()
        assert (st["seen"], st["kept"], st["since_best"], st["stopped"]) == (3, 0, 3, True)
        _raises(capi.GPE_ERR_INVALID, eng.best_params)
        _raises(capi.GPE_ERR_INVALID, eng.best_record)
        _raises(capi.GPE_ERR_INVALID, eng.restore_best)
    finally:
        eng.close()


# ---- 5. monitor ---------------------------------------------------------------------------------------------------------------------
RUN_LAYERS, RUN_N = [2, 64, 64, 64, 2], 777          # one workgroup of k_head_mix / k_seed_mix: the trajectory repeats bit for bit


def _run_engine(**kw):
    x, flat, x_bc, tgt = mc.inputs(RUN_LAYERS, RUN_N, seed=4)
    return make_engine(mc.problem(RUN_LAYERS, RUN_N), flat, x, x_bc, tgt, "auto", **kw)


def _held_out(n=301, seed=5):
    return dev(np.random.default_rng(seed).uniform(-2, 2, (n, 2)).astype(np.float32)), 16.0 / n


def test_monitor_records_equal_stop_and_look_and_follow_set_mixture():
    """A: monitor every 6 steps, run(20) (graph replays cut at the monitor steps), the couplings changed, run(10).  B, no monitor:
    run(6) and look, three times, the same change, run(6) and look.  Byte for byte; A's parameters equal those of C, which ran without
    a monitor: the monitor does not disturb training."""
    K, g2 = 6, (2.0, 5.0, -1.5)
    xm, dv = _held_out()
    a = _run_engine()
    b = _run_engine()
    c = _run_engine()
    try:
        a.bind_mixture_monitor(xm, every=K, dv=dv)
        a.run(20)
        a.set_mixture(*g2)
        a.run(10)
        recs = a.read_mixture_monitor()
        assert a.monitor_available() == 5 == len(recs) and [r["step"] for r in recs] == [6.0, 12.0, 18.0, 24.0, 30.0]
        arr = a.read_mixture_monitor_array()
        assert arr.shape == (5, len(F)) and list(arr[:, F.index("step")]) == [6.0, 12.0, 18.0, 24.0, 30.0]
        assert arr[:, F.index("energy")].tobytes() == np.array([r["energy"] for r in recs]).tobytes()
        looks = []
        for i in range(5):
            if i == 3:
                b.run(2); b.set_mixture(*g2); b.run(4)
            else:
                b.run(K)
            looks.append(b.mixture_observables(xm, dv=dv))
        for r, o in zip(recs, looks):
            assert _bytes(r) == _bytes(o), (r, o)
        # the change of couplings shows in the record behind it: the same parameters under the old couplings give another energy
        b.set_mixture(*mc.G)
        old = b.mixture_observables(xm, dv=dv)
        assert abs(old["energy"] - recs[4]["energy"]) > 1e-2 * abs(recs[4]["energy"]) and old["norm"] == recs[4]["norm"]
        c.run(20); c.set_mixture(*g2); c.run(10)
        np.testing.assert_array_equal(a.get_params(), c.get_params())
    finally:
        a.close(); b.close(); c.close()


def test_monitor_ring_keeps_the_newest_and_a_rebind_restarts():
    xm, dv = _held_out(200, 6)
    a = _run_engine()
    try:
        a.bind_mixture_monitor(xm, every=2, dv=dv, capacity=3)
        a.run(11)                                                       # records at steps 2, 4, 6, 8, 10
        assert a.monitor_available() == 5
        assert [r["step"] for r in a.read_mixture_monitor()] == [6.0, 8.0, 10.0]
        assert [r["step"] for r in a.read_mixture_monitor(3, 2)] == [8.0, 10.0]
        _raises(capi.GPE_ERR_INVALID, a.read_mixture_monitor, 0, 1)     # overwritten
        _raises(capi.GPE_ERR_INVALID, a.read_mixture_monitor, 4, 2)     # not written yet
        import ctypes                                                   # a bind the library refuses leaves the monitor and its records
        assert a.lib.gpe_mixture_monitor(a._h, ctypes.c_void_p(xm.data_ptr()), -1, None, dv, 2, 3) == capi.GPE_ERR_INVALID
        assert a.monitor_available() == 5
        a.clear_monitor()
        a.run(4)
        assert a.monitor_available() == 0 and a.read_mixture_monitor() == []
        a.bind_mixture_monitor(xm, every=3, dv=dv, capacity=3)
        a.run(3)
        recs = a.read_mixture_monitor()
        assert len(recs) == 1 and recs[0]["step"] == 18.0               # record 0 again; the optimiser step goes on counting
    finally:
        a.close()


# ---- 6. keeper ------------------------------------------------------------------------------------------------------------------------
EVERY, N_REC, LR2 = 5, 4, 0.1          # 20 steps at lr 1e-3, then 20 at an lr that wrecks the state: the best record lies inside the run


def _keeper_engine():
    e = _run_engine(lr=1e-3, sched=capi.SCHED_CONST)
    xm, dv = _held_out()
    e.bind_mixture_monitor(xm, every=EVERY, dv=dv)
    return e, xm, dv


@functools.lru_cache(maxsize=None)
def _reference_run():
    """engine B, driven from the host: the parameters behind every record, and the records; nothing here is modified later"""
    b, _, _ = _keeper_engine()
    params = []
    try:
        for half in range(2):
            if half:
                b.set_lr(LR2)
            for _ in range(N_REC):
                b.run(EVERY)
                params.append(b.get_params())
        recs, arr = b.read_mixture_monitor(), b.read_mixture_monitor_array()
    finally:
        b.close()
    for p in params:
        p.setflags(write=False)
    arr.setflags(write=False)
    return params, recs, arr


@pytest.mark.parametrize("metric", ["res_rms", "energy"])
def test_keeper_keeps_what_select_names(metric):
    params, recs, arr = _reference_run()
    vals = arr[:, F.index("res_rms_total" if metric == "res_rms" else "energy")]
    kept, kept_all, _ = keeper.select(vals)
    print(f"   {metric}: " + " ".join(f"{v:.6e}" for v in vals) + f" -> kept {kept} of {kept_all}")
    # res_rms: the best record lies strictly inside the run, so neither "keep the first" nor "keep the last" passes.  energy: this run
    # (the residual loss alone is trained) ends on its lowest energy, so there the rule must have kept some records and passed over others,
    # and must keep another record than res_rms does: the metric switch is told apart
    assert kept is not None and 1 < len(kept_all) < len(vals), (kept_all, list(vals))
    if metric == "res_rms":
        assert 0 < kept < len(vals) - 1, (kept, list(vals))
    else:
        assert kept != keeper.select(arr[:, F.index("res_rms_total")])[0]
    a, xm, dv = _keeper_engine()
    try:
        a.bind_mixture_keeper(metric)
        a.run(EVERY * N_REC)
        a.set_lr(LR2)
        a.run(EVERY * N_REC)
        np.testing.assert_array_equal(a.best_params(), params[kept])
        assert _bytes(a.best_record()) == _bytes(recs[kept])
        st = a.keeper_state()
        assert {k: st[k] for k in ("seen", "kept", "since_best")} == keeper.counters(len(vals), kept_all) and st["stopped"] is False
        np.testing.assert_array_equal(a.get_params(), params[-1])                 # the keeper did not disturb training
        a.restore_best()
        np.testing.assert_array_equal(a.get_params(), params[kept])
        back = a.mixture_observables(xm, dv=dv)
        want = dict(recs[kept], step=back["step"])                                # (the optimiser step went on counting)
        assert _bytes(back) == _bytes(want) and back["step"] == 2.0 * EVERY * N_REC
    finally:
        a.close()


def test_keeper_patience_stops_at_the_record_select_names_and_a_rebind_restarts_it():
    params, recs, arr = _reference_run()
    vals = arr[:, F.index("res_rms_total")]
    kept, kept_all, stop = keeper.select(vals, patience=2)
    assert stop is not None and stop < len(vals) - 1, (stop, list(vals))
    a, xm, dv = _keeper_engine()
    try:
        a.bind_mixture_keeper("res_rms", patience=2)
        a.run(EVERY * N_REC)
        a.set_lr(LR2)
        a.run(EVERY * N_REC)
        assert a.stop_state() == (True, int(recs[stop]["step"])) and a.keeper_state()["stopped"] is True
        np.testing.assert_array_equal(a.get_params(), params[stop])
        kept_s = keeper.select(vals[:stop + 1], patience=2)[0]
        np.testing.assert_array_equal(a.best_params(), params[kept_s])
        a.bind_mixture_monitor(xm, every=EVERY, dv=dv)                            # a re-bind: armed, nothing kept
        st = a.keeper_state()
        assert (st["seen"], st["kept"], st["since_best"]) == (0, 0, 0)
        _raises(capi.GPE_ERR_INVALID, a.best_params)
        a.clear_monitor()                                                         # clearing the monitor disarms the keeper
        _raises(capi.GPE_ERR_STATE, a.keeper_state)
    finally:
        a.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    xs = dev(np.zeros((8, 2), np.float32))
    scalar = Engine(GPEConfig(layers=[2, 64, 64, 1]))
    try:
        for call in (lambda: scalar.mixture_observables(xs), lambda: scalar.bind_mixture_monitor(xs, 2), lambda: scalar.read_mixture_monitor(0, 1),
                     lambda: scalar.bind_mixture_keeper("res_rms")):
            _raises(capi.GPE_ERR_STATE, call)
        import ctypes as C
        assert scalar.lib.gpe_mixture_keeper_read(scalar._h, None, 0, None, None, None, None, None) == capi.GPE_ERR_STATE
        assert scalar.lib.gpe_mixture_keeper(scalar._h, capi.KEEP_NONE, 0.0, 0) == capi.GPE_ERR_STATE
        assert scalar.lib.gpe_mixture_monitor(scalar._h, None, 0, None, C.c_float(0.0), 0, 0) == capi.GPE_ERR_STATE
    finally:
        scalar.close()
    mp, x, flat, _, _, _ = mc.case("fused_2d_64x3_N37")
    eng = make_engine(mp, flat, x)
    try:
        _raises(capi.GPE_ERR_INVALID, eng.bind_mixture_keeper, "res_rms")          # no monitor bound
        eng.bind_mixture_monitor(dev(x), every=2)
        _raises(capi.GPE_ERR_INVALID, eng.bind_mixture_keeper, "res_rms", -1.0)
        _raises(capi.GPE_ERR_INVALID, eng.bind_mixture_keeper, "res_rms", 0.0, -1)
        assert eng.lib.gpe_mixture_keeper(eng._h, 7, 0.0, 0) == capi.GPE_ERR_INVALID
        _raises(capi.GPE_ERR_STATE, eng.read_monitor, 0, 1)                        # the scalar reads keep refusing a mixture
        eng.bind_mixture_keeper("energy")
        rec = capi.gpe_observables()
        import ctypes as C
        assert eng.lib.gpe_keeper_read(eng._h, None, 0, C.byref(rec), None, None, None, None) == capi.GPE_ERR_STATE
        eng.clear_keeper()
        _raises(capi.GPE_ERR_STATE, eng.keeper_state)
    finally:
        eng.close()
    unbound = Engine(config(mp))
    try:
        _raises(capi.GPE_ERR_STATE, unbound.mixture_observables)                   # NULL points before bind_points
    finally:
        unbound.close()


def test_keeper_refuses_an_engine_with_a_communicator():
    mp, x, flat, _, _, _ = mc.case("fused_2d_64x3_N37")
    eng = make_engine(mp, flat, x)
    try:
        eng.comm_init(0, 1)
        eng.bind_mixture_monitor(dev(x), every=2)
        _raises(capi.GPE_ERR_INVALID, eng.bind_mixture_keeper, "res_rms")
    finally:
        eng.close()


# ---- 8. a short training run ------------------------------------------------------------------------------------------------------------
def test_short_immiscible_run_keeps_the_lowest_energy_and_the_overlap_falls():
    """1D, g_12^2 > g_11 g_22, trained with the mixture energy term for 300 steps; monitor on a finer grid every 10 steps, keeper on the
    energy.  The start is a random network whose second output row is nearly the first (u_2 = 0.9 u_1 + 0.1 of its own row): the
    densities start almost proportional, overlap close to 1, and the immiscible couplings drive them apart."""
    layers, N, L = [1, 32, 32, 2], 256, 6.0
    x = np.linspace(-L, L, N, dtype=np.float32).reshape(-1, 1)
    xm = np.linspace(-L, L, 601, dtype=np.float32).reshape(-1, 1)
    dx, dvm = 2 * L / (N - 1), 2 * L / 600
    _, flat, _, _ = mc.inputs(layers, N, seed=3)
    params = go.unflatten(flat.astype(np.float64), layers)
    W, b = params[-1]
    W[1], b[1] = 0.9 * W[0] + 0.1 * W[1], 0.9 * b[0] + 0.1 * b[1]
    flat = go.flatten(params).astype(np.float32)
    cfg = GPEConfig(layers=layers, kinetic_coeff=0.5, pot_scale=0.5, dx=dx, w_pde=1.0, w_bc=0.0, w_norm=20.0, lr=5e-3, clip_norm=1.0,
                    sched=capi.SCHED_CONST, mixture=True, mix_g=(4.0, 4.0, 12.0), mix_norm=(0.5, 0.5), n_global=N)
    eng = Engine(cfg)
    try:
        eng.set_params(flat)
        eng.bind_points(dev(x))
        eng.set_mixture_energy(1.0)
        eng.bind_mixture_monitor(dev(xm), every=10, dv=dvm)
        eng.bind_mixture_keeper("energy")
        eng.run(300)
        recs = eng.read_mixture_monitor()
        best = eng.best_record()
    finally:
        eng.close()
    en = [r["energy"] for r in recs]
    print("   energy " + " ".join(f"{v:.5f}" for v in en) + "\n   overlap " + " ".join(f"{r['overlap']:.4f}" for r in recs))
    assert len(recs) == 30 and all(np.isfinite(_flat(r)).all() for r in recs)
    assert all(best["energy"] <= v for v in en) and _bytes(best) in [_bytes(r) for r in recs]
    assert recs[0]["overlap"] > 0.5 and recs[-1]["overlap"] < recs[0]["overlap"] and best["overlap"] < recs[0]["overlap"]
