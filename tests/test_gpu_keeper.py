"""The keeper (include/gpe_hip.h: gpe_bind_keeper / gpe_keeper_read / gpe_keeper_restore): the best parameters by the held-out monitor,
kept on the device, and the patience stop.

Reference: always a SECOND engine B driven from the host -- B.run(every), B.get_params(), repeated; its records from B.read_monitor();
the kept index from gpe_pinn.keeper.select on B's records -- never engine A's own keeper.  One GPU repeats a trajectory and its monitor
records bit for bit (README "Reproducibility", tests/test_gpu_observables.py::test_monitor_records_equal_stop_and_look), so every
comparison is exact: np.array_equal on parameters, byte equality on records.

Every run is 60 steps at lr 1e-3, then set_lr(lr2) with lr2 large enough to wreck the state, then 60 more: the best record lies
strictly inside the run, so neither "keep the first" nor "keep the last" passes.  That is asserted on B alone before anything is
compared.  B's runs are computed once per (case, lr2) and shared."""
import functools

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import capi, keeper
from oracle import gpe_oracle as go
from tests.test_gpu_parity import PATHS, _inputs, _scale, cfg_from_problem

pytestmark = pytest.mark.gpu

EVERY, N_REC = 10, 6                 # monitor cadence; records per half of a run
LR1 = 1e-3

# name: (Problem kwargs, path, lr2) -- lr2 chosen per case so that B's best record is neither the first nor the last (read once from
# B's numbers on the GPU; asserted in every test through _interior)
CASES = {
    "1d_32x2_fused_single_wg": (dict(layers=[1, 32, 32, 1], gamma=1.0, dx=12.0 / 255), "fused", 0.1),
    "2d_64x4_pipelined": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=36.0 / 256), "fused", 0.1),
    "2d_100x2_padded": (dict(layers=[2, 100, 100, 1], gamma=50.0, dx=36.0 / 256), "fused", 0.1),
    "2d_128x3_multi_wg_update": (dict(layers=[2, 128, 128, 128, 1], gamma=50.0, dx=36.0 / 256), "fused", 0.1),
    # forced onto the generic layer-by-layer set.  Widths that are no multiple of 64 on purpose: for multiples of 64 that set forms the
    # weight gradient with its split-K MFMA kernels, which add their partial products with float atomics -- such a trajectory does not
    # repeat bit for bit (two engines of [2,64,64,64,1] on this path differ in the sixth digit of res_rms after 30 steps), so no second
    # engine could be compared exactly.  At width 40 every kernel of the set adds in a fixed order (three runs: the same twelve digits).
    "2d_40x3_generic": (dict(layers=[2, 40, 40, 40, 1], gamma=50.0, dx=36.0 / 256), "generic", 0.1),
}
ENERGY_CASE = "2d_100x2_padded"             # energy keeps record 5 there, res_rms record 1
SEQ_CASE = "1d_32x2_fused_single_wg"        # res_rms falls over six records with unequal gains, then rises: min_delta and patience = 2
MAIN_CASE = "2d_64x4_pipelined"


def _bytes(d):
    return np.array([v for k in d for v in (d[k] if isinstance(d[k], list) else [d[k]])], np.float64).tobytes()


def _raises(code, fn, *args, **kw):
    with pytest.raises(gpe_pinn.GPEError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


def _monitor_points(d):
    rng = np.random.default_rng(11)
    xm = (np.sort(rng.uniform(-6, 6, (256, 1)), axis=0) if d == 1 else rng.uniform(-3, 3, (256, 2))).astype(np.float32)
    return torch.as_tensor(xm, device="cuda"), (12.0 if d == 1 else 36.0) / 256


def _engine(name, sampler=True, monitor=True, **cfg_kw):
    """engine of the case at its start parameters: 2D on a 16 x 16 sampler redrawn every 5 steps (sampler=False: its draw 0 as fixed
    points), 1D on 256 fixed points; 256 held-out monitor points every EVERY steps"""
    kw, path, _ = CASES[name]
    d = kw["layers"][0]
    x, flat, _ = _inputs(kw, 256, scale=_scale(kw))
    cfg = cfg_from_problem(go.Problem(**kw), lr=LR1, sched=capi.SCHED_CONST, path=PATHS[path], **cfg_kw)
    cfg.w_bc = 0.0
    eng = gpe_pinn.Engine(cfg)
    assert eng.active_path == PATHS[path]
    eng.set_params(flat)
    if d == 1:
        eng.bind_points(torch.as_tensor(x, device="cuda"))
    elif sampler:
        eng.bind_sampler(-3.0, 3.0, (16, 16), every=5, seed=7)
    else:
        eng.bind_points(torch.as_tensor(gpe_pinn.sampler.stratified_points(-3.0, 3.0, (16, 16), 7, 0), device="cuda"))
    if monitor:
        xm, dv = _monitor_points(d)
        eng.bind_monitor(xm, every=EVERY, dv=dv)
    return eng


@functools.lru_cache(maxsize=None)
def _reference(name, lr2):
    """engine B: (parameters after every record, the records as dicts, the records as an array); nothing here is modified later"""
    b = _engine(name)
    params = []
    for half in range(2):
        if half:
            b.set_lr(lr2)
        for _ in range(N_REC):
            b.run(EVERY)
            params.append(b.get_params())
    recs, arr = b.read_monitor(), b.read_monitor_array()
    b.close()
    for p in params:
        p.setflags(write=False)
    arr.setflags(write=False)
    assert len(recs) == 2 * N_REC and [r["step"] for r in recs] == [float(EVERY * (i + 1)) for i in range(2 * N_REC)]
    return params, recs, arr


def _column(arr, metric):
    return arr[:, gpe_pinn.Engine.OBSERVABLE_FIELDS.index(metric)]


def _interior(name, lr2, metric="res_rms", **sel):
    """select on B's records; the kept index must lie strictly inside the run"""
    params, recs, arr = _reference(name, lr2)
    vals = _column(arr, metric)
    kept, kept_all, stop = keeper.select(vals, **sel)
    print(f"   {name} lr2 {lr2} {metric}: " + " ".join(f"{v:.6e}" for v in vals) + f" -> kept {kept} of {kept_all}, stop {stop}")
    assert kept is not None and 0 < kept < len(vals) - 1, (kept, list(vals))
    return params, recs, vals, kept, kept_all, stop


def _run_a(name, lr2, **keeper_kw):
    a = _engine(name)
    a.bind_keeper(**keeper_kw)
    a.run(EVERY * N_REC)
    a.set_lr(lr2)
    a.run(EVERY * N_REC)
    return a


def _check_kept(a, params, recs, kept, kept_all, n_seen):
    np.testing.assert_array_equal(a.best_params(), params[kept])
    assert _bytes(a.best_record()) == _bytes(recs[kept])
    st = a.keeper_state()
    assert {k: st[k] for k in ("seen", "kept", "since_best")} == keeper.counters(n_seen, kept_all), st


# ---- 1. the right step, exactly, per kernel family -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_keeps_the_parameters_of_the_best_record(name):
    lr2 = CASES[name][2]
    params, recs, vals, kept, kept_all, _ = _interior(name, lr2)
    a = _run_a(name, lr2, metric="res_rms")
    _check_kept(a, params, recs, kept, kept_all, len(vals))
    assert a.keeper_state()["stopped"] is False and a.stop_state() == (False, 0)
    assert a.n_params == go.param_count(CASES[name][0]["layers"]) == a.best_params().size
    np.testing.assert_array_equal(a.get_params(), params[-1])            # the keeper did not disturb training
    assert _bytes(a.read_monitor()[-1]) == _bytes(recs[-1])
    a.close()


# ---- 2. the other metric ------------------------------------------------------------------------------------------------------------
def test_energy_metric():
    name = ENERGY_CASE
    lr2 = CASES[name][2]
    params, recs, vals, kept, kept_all, _ = _interior(name, lr2, metric="energy")
    kept_rms = keeper.select(_column(_reference(name, lr2)[2], "res_rms"))[0]
    if kept == kept_rms:
        print(f"   energy and res_rms keep the same record ({kept}) in this run: the metric switch is not told apart here")
    a = _run_a(name, lr2, metric="energy")
    _check_kept(a, params, recs, kept, kept_all, len(vals))
    np.testing.assert_array_equal(a.get_params(), params[-1])
    a.close()


# ---- 3. min_delta ---------------------------------------------------------------------------------------------------------------------
def test_min_delta_between_two_successive_gains():
    name = SEQ_CASE
    lr2 = CASES[name][2]
    params, recs, vals, kept0, kept_all0, _ = _interior(name, lr2)
    gains = sorted(vals[i] - vals[j] for i, j in zip(kept_all0[:-1], kept_all0[1:]))
    assert len(gains) >= 2 and gains[0] < gains[-1], gains
    min_delta = 0.5 * (gains[0] + gains[1])                                # above the smallest gain of the plain run, below the next
    kept, kept_all, _ = keeper.select(vals, min_delta=min_delta)
    print(f"   gains {gains} min_delta {min_delta:.6e}: kept {kept_all} (min_delta = 0: {kept_all0})")
    assert kept_all != kept_all0 and kept is not None and 0 < kept < len(vals) - 1
    a = _run_a(name, lr2, metric="res_rms", min_delta=min_delta)
    _check_kept(a, params, recs, kept, kept_all, len(vals))
    a.close()


# ---- 4. the patience stop ---------------------------------------------------------------------------------------------------------
def test_patience_stops_the_optimiser_at_the_record_select_names():
    name = SEQ_CASE
    lr2 = CASES[name][2]
    params, recs, vals, _, _, _ = _interior(name, lr2)
    stop = keeper.select(vals, patience=2)[2]
    assert stop is not None and N_REC <= stop < len(vals) - 1, (stop, list(vals))       # in the wrecked half, with records left behind it
    a = _run_a(name, lr2, metric="res_rms", patience=2)
    assert a.stop_state() == (True, int(recs[stop]["step"]))
    assert a.keeper_state()["stopped"] is True
    np.testing.assert_array_equal(a.get_params(), params[stop])
    a.run(30)                                                               # frozen: further steps leave the parameters untouched
    np.testing.assert_array_equal(a.get_params(), params[stop])
    # B trained on behind the stop; A's records there repeat the one at the stop (frozen parameters, fixed monitor points)
    n_seen = len(vals) + 30 // EVERY
    kept, kept_all, stop_a = keeper.select(list(vals[:stop + 1]) + [vals[stop]] * (n_seen - stop - 1), patience=2)
    assert stop_a == stop and 0 < kept < stop
    _check_kept(a, params, recs, kept, kept_all, n_seen)
    assert all(_bytes(r) == _bytes(recs[stop]) for r in a.read_monitor()[stop:])
    # gpe_reset_optimizer clears the stop; the kept set survives it
    best = a.best_params()
    a.reset_optimizer(LR1)
    assert a.stop_state() == (False, 0)
    np.testing.assert_array_equal(a.best_params(), best)
    assert a.keeper_state()["kept"] == len(kept_all)
    a.close()


def test_loss_based_stop_alone_is_unchanged():
    """stop_tol with a monitor and no keeper: fires at step 1 (every loss is below 1e30), the parameters freeze there, and nothing
    about a keeper exists"""
    name = MAIN_CASE
    a = _engine(name, stop_tol=1e30)
    c = _engine(name)
    a.run(25)
    c.run(1)
    assert a.stop_state() == (True, 1)
    np.testing.assert_array_equal(a.get_params(), c.get_params())
    assert [r["step"] for r in a.read_monitor()] == [1.0, 1.0]
    _raises(capi.GPE_ERR_STATE, a.keeper_state)
    a.close(); c.close()


# ---- 5. restore -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d_64x4_pipelined", "2d_128x3_multi_wg_update"])
def test_restore_best_and_step_on(name):
    """after restore_best() one step equals the step of a fresh engine given the kept parameters (and A's Adam state, lr): loss, mu and
    gradient bit for bit -- stale packed weight copies would show in all three.  Fixed points: the fresh engine sees the same set."""
    lr2 = CASES[name][2]
    a = _engine(name, sampler=False)
    a.bind_keeper()
    a.run(EVERY * N_REC)
    a.set_lr(lr2)
    a.run(EVERY * N_REC)
    best = a.best_params()
    assert a.keeper_state()["kept"] >= 1 and not np.array_equal(best, a.get_params())
    a.restore_best()
    np.testing.assert_array_equal(a.get_params(), best)
    m, v, step = a.get_adam_state()
    assert step == 2 * EVERY * N_REC                                        # the optimiser state stayed
    f = _engine(name, sampler=False, monitor=False)
    f.set_params(best)
    f.set_adam_state(m, v, step)
    f.set_lr(lr2)
    sa, sf = a.step(), f.step()
    assert sa["step"] == sf["step"] == step + 1
    for k in ("loss", "mu", "pde", "norm", "grad_norm"):
        assert np.float64(sa[k]).tobytes() == np.float64(sf[k]).tobytes(), (k, sa[k], sf[k])
    np.testing.assert_array_equal(a.get_grad(), f.get_grad())
    np.testing.assert_array_equal(a.best_params(), best)                    # restoring and stepping on left the kept set alone
    a.close(); f.close()


# ---- 6. non-finite records --------------------------------------------------------------------------------------------------------
def test_non_finite_records_are_counted_never_kept_and_run_out_the_patience():
    kw = dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=36.0 / 256, potential=go.POT_PRECOMPUTED)
    x, flat, _ = _inputs(kw, 256, scale=_scale(kw))
    cfg = cfg_from_problem(go.Problem(**kw), lr=LR1, sched=capi.SCHED_CONST)
    cfg.w_bc = 0.0
    a = gpe_pinn.Engine(cfg)
    a.set_params(flat)
    a.bind_points(torch.as_tensor(x, device="cuda"), V=0.5 * (x.astype(np.float64) ** 2).sum(axis=1))
    xm, dv = _monitor_points(2)
    a.bind_monitor(xm, every=EVERY, V=np.full(256, np.inf, np.float32), dv=dv)
    a.bind_keeper(metric="res_rms", patience=3)
    a.run(2 * EVERY)
    assert a.keeper_state() == dict(seen=2, kept=0, since_best=2, stopped=False) and a.stop_state() == (False, 0)
    assert not any(np.isfinite(r["res_rms"]) for r in a.read_monitor())
    assert "nothing kept" in _raises(capi.GPE_ERR_INVALID, a.best_params)
    _raises(capi.GPE_ERR_INVALID, a.best_record)
    _raises(capi.GPE_ERR_INVALID, a.restore_best)
    a.run(2 * EVERY)
    assert a.keeper_state() == dict(seen=4, kept=0, since_best=4, stopped=True)
    assert a.stop_state() == (True, 3 * EVERY)                              # at the third record
    assert keeper.select([r["res_rms"] for r in a.read_monitor()], patience=3) == (None, [], 2)
    a.close()


# ---- 7. lifetime and refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_keeper_that_was_there():
    name = MAIN_CASE
    lr2 = CASES[name][2]
    a = _engine(name, monitor=False)
    assert "monitor" in _raises(capi.GPE_ERR_INVALID, a.bind_keeper)        # no monitor bound
    _raises(capi.GPE_ERR_STATE, a.keeper_state)
    a.close()
    params, recs, vals, kept, kept_all, _ = _interior(name, lr2)
    a = _run_a(name, lr2, metric="res_rms")
    _raises(capi.GPE_ERR_INVALID, a.bind_keeper, min_delta=-1e-3)
    _raises(capi.GPE_ERR_INVALID, a.bind_keeper, min_delta=float("nan"))
    _raises(capi.GPE_ERR_INVALID, a.bind_keeper, patience=-1)
    assert a.lib.gpe_bind_keeper(a._h, 7, 0.0, 0) == capi.GPE_ERR_INVALID   # no such metric
    with pytest.raises(ValueError):
        a.bind_keeper(metric="mu")
    _check_kept(a, params, recs, kept, kept_all, len(vals))                 # every failed bind left the keeper and its kept set
    a.comm_init(0, 1)
    assert "communicator" in _raises(capi.GPE_ERR_INVALID, a.bind_keeper)
    _check_kept(a, params, recs, kept, kept_all, len(vals))
    a.close()


def test_monitor_rebind_resets_and_monitor_clear_disarms():
    name = MAIN_CASE
    a = _engine(name)
    a.bind_keeper()
    a.run(2 * EVERY)
    assert a.keeper_state()["seen"] == 2 and a.keeper_state()["kept"] >= 1
    # setters, reset_optimizer and a bind of points leave the keeper alone
    best, st = a.best_params(), a.keeper_state()
    a.set_gamma(40.0); a.set_params(best); a.reset_optimizer(LR1)
    a.bind_sampler(-3.0, 3.0, (16, 16), every=5, seed=8)
    assert a.keeper_state() == st
    np.testing.assert_array_equal(a.best_params(), best)
    # a new monitor: "nothing kept", still armed
    xm, dv = _monitor_points(2)
    a.bind_monitor(xm + 0.01, every=EVERY, dv=dv)
    assert a.keeper_state() == dict(seen=0, kept=0, since_best=0, stopped=False)
    _raises(capi.GPE_ERR_INVALID, a.best_params)
    a.run(EVERY)
    assert a.keeper_state()["seen"] == 1 and a.keeper_state()["kept"] == 1
    np.testing.assert_array_equal(a.best_params(), a.get_params())
    # re-arming starts again as well; clearing the keeper or the monitor disarms it
    a.bind_keeper(metric="energy")
    assert a.keeper_state() == dict(seen=0, kept=0, since_best=0, stopped=False)
    a.clear_keeper()
    _raises(capi.GPE_ERR_STATE, a.keeper_state)
    a.bind_keeper()
    a.clear_monitor()
    _raises(capi.GPE_ERR_STATE, a.keeper_state)
    _raises(capi.GPE_ERR_STATE, a.restore_best)
    a.run(EVERY)                                                            # nothing left to launch
    a.synchronize()
    a.close()


def test_run_with_a_keeper_does_not_wait_for_the_device():
    """gpe_run with monitor and keeper returns while its steps are still running: 100 steps at 262 144 points are ~70 ms of kernels and
    ~1 000 launches (a few ms of host time); a keeper that synchronised at its records would return only behind the last one (step
    100 is a monitor step).  An event recorded behind the run must still be pending when run() returns."""
    kw = dict(layers=[2, 64, 64, 64, 64, 1], gamma=50.0, dx=36.0 / 262144)
    x, flat, _ = _inputs(kw, 262144, scale=_scale(kw))
    cfg = cfg_from_problem(go.Problem(**kw), lr=LR1, sched=capi.SCHED_CONST)
    cfg.w_bc = 0.0
    a = gpe_pinn.Engine(cfg)
    a.set_params(flat)
    a.bind_points(torch.as_tensor(x, device="cuda"))
    xm, dv = _monitor_points(2)
    a.bind_monitor(xm, every=EVERY, dv=dv)
    a.bind_keeper(patience=1000)
    a.run(EVERY)                                                            # warm: first launches load the code objects
    a.synchronize()
    ev = torch.cuda.Event()
    a.run(10 * EVERY)
    ev.record()
    pending = not ev.query()
    a.synchronize()
    assert pending, "run() returned only after its last step had finished"
    assert a.keeper_state()["seen"] == 11
    a.close()


# ---- 8. a frozen orthogonality state from the kept set ---------------------------------------------------------------------------
def test_frozen_state_from_the_best_set():
    name = MAIN_CASE
    lr2 = CASES[name][2]
    ground = _run_a(name, lr2, metric="res_rms")
    best = ground.best_params()
    assert not np.array_equal(best, ground.get_params())
    exc = _engine(name, monitor=False, w_orth=5.0)
    exc.bind_orth_state(0, ground, which="best")
    v_best = exc.orth_values(0).cpu().numpy()
    exc.bind_orth_state(0, best)
    np.testing.assert_array_equal(v_best, exc.orth_values(0).cpu().numpy())
    exc.bind_orth_state(0, ground)                                          # the default stays the last set
    v_last = exc.orth_values(0).cpu().numpy()
    exc.bind_orth_state(0, ground.get_params())
    np.testing.assert_array_equal(v_last, exc.orth_values(0).cpu().numpy())
    assert not np.array_equal(v_last, v_best)
    with pytest.raises(ValueError):
        exc.bind_orth_state(0, best, which="best")
    ground.close(); exc.close()
