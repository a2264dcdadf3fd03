"""The device-resident L-BFGS under the held-out monitor and the keeper (include/gpe_hip.h: gpe_lbfgs_monitor, gpe_lbfgs_point;
csrc/gpe_lbfgs.h: k_lbfgs_view, k_lbfgs_unview; csrc/gpe_lbfgs_rules.h: lbfgs_judged_at_start, lbfgs_freeze): records are of the JUDGED POINT -- theta without a line search and in a frozen state,
the start point of the running search under strong Wolfe -- the run itself is not disturbed, and the keeper's patience freezes it with
code 4.

Reference: always OTHER engines driven from the host from the same start -- lbfgs_run(every), then observables() on the held-out points
(stop-and-look), or lbfgs_point() of a fresh engine handed to a third one by set_params -- never engine A's own monitor.  The L-BFGS
kernels repeat bit for bit (tests/test_gpu_lbfgs.py::test_bit_repeatability), the observe chain has no atomics and N = 256 training
points are one chunk of the generic weight-gradient kernel, so every comparison is exact: byte equality on records, np.array_equal on
parameters and histories.  No tolerance is used.

Engines: tests/test_gpu_lbfgs.make_engine (256 points, the PDE residual alone) on the cells below; the strong-Wolfe runs are the
physics run of tests/test_gpu_lbfgs_ls._whole_run at LS_LR, where the fp64 reference tests/lbfgs_ls_ref.py on the fp64 oracle is in the
MIDDLE of a search at monitor ticks (asserted here on the CPU before any device result is compared).

The generic cell keeps the issue's [2,64,64,64,1]: at widths that are multiples of 64 the generic set forms the weight gradient with
g_bwd_weight_mfma, split-K over chunks of points added with float atomics, and with the default 32 points per chunk 256 points are 8
chunks -- such a run does not repeat bit for bit.  With GPE_GEN_MIN_CHUNK=256 (an existing switch, read at engine creation) they are ONE
chunk: every element of the gradient receives one addition, and the run repeats."""
import functools

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import GPEError, capi, keeper
from tests import lbfgs_ls_cases as cases
from tests import lbfgs_ls_ref as ls_
from tests import lbfgs_ref as lr_
from tests import test_gpu_lbfgs as base
from tests import test_gpu_lbfgs_ls as lsb
from tests.test_gpu_lbfgs import SHAPES, make_engine
from tests.test_gpu_lbfgs_ls import ls_engine

pytestmark = pytest.mark.gpu

EVERY = 3
# Strong-Wolfe runs: the smallest power of two at which the fp64 reference ALONE (no device involved) is in the middle of a search --
# bracket or zoom phase -- at a monitor tick, with the decision margins of all its 24 leading ticks above 1e-3 so that the device takes
# the same decisions: at lr 4 the phases are a a b a z a b a z z a a z a z ... (mid-search at tick counts 3, 9, 15); at 0.5, 1 and 2 every
# tick whose count is a multiple of 3 accepts a point.
LS_LR = 4.0
FROZEN_KEEPER = 4
MIX = dict(mixture=True, mix_g=(1.0, 1.0, 0.5), mix_norm=(0.5, 0.5))
# name: (layers, path, further configuration, lr of the run without a line search)
CELLS = {
    "fused_1d": (SHAPES["P1153"][0], gpe_pinn.PATH_AUTO, {}, 0.05),
    "fused_2d": ([2, 64, 64, 64, 1], gpe_pinn.PATH_AUTO, {}, 0.05),            # packed weight copies
    "generic_2d": ([2, 64, 64, 64, 1], gpe_pinn.PATH_GENERIC, {}, 0.05),       # none
    "padded_2d": ([2, 72, 72, 1], gpe_pinn.PATH_AUTO, {}, 0.05),               # hidden width 72 -> 128: ld != P_user
    "mixture_1d": ([1, 32, 32, 2], gpe_pinn.PATH_AUTO, MIX, 0.05),             # the mixture record kind
}


def _bytes(d):
    return np.array([v for k in d for v in (np.ravel(d[k]).tolist() if isinstance(d[k], (list, tuple)) else [d[k]])], np.float64).tobytes()


def _raises(code, fn, *args, **kw):
    with pytest.raises(GPEError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, (ei.value.code, str(ei.value))


def _held_out(d):
    """53 points that are not training points (another generator), and their quadrature weight"""
    x = np.random.default_rng(91).uniform(-3, 3, (53, d)).astype(np.float32)
    return torch.as_tensor(x, device="cuda"), 6.0 ** d / 53


@pytest.fixture(autouse=True)
def _one_chunk(monkeypatch):
    monkeypatch.setenv("GPE_GEN_MIN_CHUNK", "256")                                        # (module docstring; generic set only)


def _cell_engine(cell, line_search=None, lr=None, **cfg):
    layers, path, kw, lr0 = CELLS[cell]
    eng = make_engine(layers, path, **kw)
    cfg = dict(dict(history=5, tolerance_grad=1e-30), **cfg)
    eng.lbfgs_config(lr0 if lr is None else lr, line_search=line_search, **cfg)
    return eng


def _bind(eng, every=EVERY, keeper_kw=None):
    x, dv = _held_out(eng.cfg.layers[0])
    (eng.bind_mixture_monitor if eng.cfg.mixture else eng.bind_monitor)(x, every=every, dv=dv)
    if keeper_kw is not None:
        (eng.bind_mixture_keeper if eng.cfg.mixture else eng.bind_keeper)(**keeper_kw)
    return eng


def _look(eng):
    x, dv = _held_out(eng.cfg.layers[0])
    return (eng.mixture_observables if eng.cfg.mixture else eng.observables)(x, dv=dv)


def _records(eng):
    return eng.read_mixture_monitor() if eng.cfg.mixture else eng.read_monitor()


def _column(eng, metric):
    if eng.cfg.mixture:
        name = "res_rms_total" if metric == "res_rms" else metric
        return eng.read_mixture_monitor_array()[:, eng.MIXTURE_OBSERVABLE_FIELDS.index(name)]
    return eng.read_monitor_array()[:, eng.OBSERVABLE_FIELDS.index(metric)]


def _state(eng):
    """everything a run leaves behind, for exact comparison"""
    return eng.get_params(), eng.lbfgs_read(), eng.lbfgs_ls_read(), eng.lbfgs_history()


def _same_state(a, b, what=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what)
    assert _bytes(a[1]) == _bytes(b[1]), (what, a[1], b[1])
    assert a[2] == b[2], (what, a[2], b[2])
    for u, v in zip(a[3], b[3]):
        np.testing.assert_array_equal(u, v, err_msg=what)


# ---- 1. no line search: records equal stop-and-look, the run is not disturbed -------------------------------------------------------------
@pytest.mark.parametrize("cell", list(CELLS))
def test_records_equal_stop_and_look(cell):
    a = _bind(_cell_engine(cell))
    a.lbfgs_monitor(True)
    a.lbfgs_run(4 * EVERY)
    recs = _records(a)
    assert len(recs) == 4
    b = _cell_engine(cell)
    for j in range(4):
        b.lbfgs_run(EVERY)
        np.testing.assert_array_equal(b.lbfgs_point(), b.get_params())                   # no line search: the judged point is theta
        want = _look(b)
        assert _bytes(recs[j]) == _bytes(want), (cell, j, recs[j], want)
    c = _cell_engine(cell)
    c.lbfgs_run(4 * EVERY)
    _same_state(_state(a), _state(c), cell)
    assert a.lbfgs_read()["n_iter"] == 4 * EVERY and a.lbfgs_read()["frozen"] == 0
    assert len({_bytes(r) for r in recs}) == 4                                           # the state moved between the records
    for e in (a, b, c):
        e.close()


# ---- 2. strong Wolfe: the record is of the accepted point ------------------------------------------------------------------------------
LS_RECORDS = 6


@functools.lru_cache(maxsize=None)
def _ls_reference():
    """the fp64 reference alone on the fp64 oracle, LS_RECORDS * EVERY ticks: theta and theta0 after every tick"""
    flat, fun, factory, mse = lsb._whole_run("physics")
    outs = ls_.run_flat(ls_.LbfgsLsRef(flat, LS_LR, 100), fun, LS_RECORDS * EVERY)
    return outs


def _ls_fresh(monitor=False, keeper_kw=None):
    flat, fun, factory, mse = lsb._whole_run("physics")
    eng = factory()
    eng.lbfgs_config(LS_LR, history=100, line_search="strong_wolfe", c1=lsb.C1, c2=lsb.C2)
    if monitor:
        _bind(eng, keeper_kw=keeper_kw)
        eng.lbfgs_monitor(True)
    return eng


@functools.lru_cache(maxsize=None)
def _ls_points():
    """For every record j a FRESH engine run 3 (j + 1) ticks unobserved: (judged point p_j, theta q_j, state); nothing here is modified"""
    out = []
    for j in range(LS_RECORDS):
        b = _ls_fresh()
        b.lbfgs_run(EVERY * (j + 1))
        st = _state(b)
        p = b.lbfgs_point()
        _same_state(_state(b), st, f"lbfgs_point wrote something (record {j})")
        b.close()
        p.setflags(write=False)
        out.append((p, st[0], st))
    return out


def test_strong_wolfe_records_are_of_the_accepted_point():
    # on the CPU, before anything of the device is compared: the reference sits at a trial point, in the middle of a search, at a record
    outs = _ls_reference()
    at_records = [outs[EVERY * (j + 1) - 1] for j in range(LS_RECORDS)]
    mid = [j for j, o in enumerate(at_records) if o["phase"] in ("bracket", "zoom") and (o["theta"] != o["theta0"]).any()]
    print(f"   reference phases at the records: {[o['phase'] for o in at_records]}; all: {[o['phase'] for o in outs]}")
    assert mid, [o["phase"] for o in outs]
    a = _ls_fresh(monitor=True)
    a.lbfgs_run(LS_RECORDS * EVERY)
    recs = _records(a)
    assert len(recs) == LS_RECORDS
    pts = _ls_points()
    differ = [j for j, (p, q, _) in enumerate(pts) if (p != q).any()]
    print(f"   records whose judged point is not theta: {differ}; device phases at the records: {[st[2]['phase'] for _, _, st in pts]}")
    assert differ and any(pts[j][2][2]["phase"] in ("bracket", "zoom") for j in differ)
    flat, fun, factory, mse = lsb._whole_run("physics")
    c = factory()
    for j, (p, q, _) in enumerate(pts):
        c.set_params(p)
        want = _look(c)
        assert _bytes(recs[j]) == _bytes(want), (j, recs[j], want)
        if j in differ:                                                                  # and NOT of theta where the two differ
            c.set_params(q)
            assert _bytes(recs[j]) != _bytes(_look(c)), j
    c.close()
    _same_state(_state(a), pts[-1][2], "the monitor disturbed the run")
    a.close()


def test_lbfgs_point_is_not_destructive_and_is_the_searchs_start_point():
    pts = _ls_points()
    for j in range(LS_RECORDS - 1):
        b = _ls_fresh()
        b.lbfgs_run(EVERY * (j + 1))
        np.testing.assert_array_equal(b.lbfgs_point(), pts[j][0])
        b.lbfgs_run(EVERY)                                                               # goes on as an engine that was never asked
        _same_state(_state(b), pts[j + 1][2], f"after lbfgs_point at record {j}")
        b.close()
    # independently: gpe_lbfgs_line_search ends a running search by putting theta back to its start point
    for j in range(LS_RECORDS):
        d = _ls_fresh()
        d.lbfgs_run(EVERY * (j + 1))
        assert d.lib.gpe_lbfgs_line_search(d._h, 1, lsb.C1, lsb.C2, 25) == capi.GPE_OK
        np.testing.assert_array_equal(d.get_params(), pts[j][0], err_msg=f"record {j}")
        d.close()


# ---- 3. the keeper keeps what keeper.select names ---------------------------------------------------------------------------------------
def _judged_point_at(make, ticks):
    b = make()
    b.lbfgs_run(ticks)
    p = b.lbfgs_point()
    b.close()
    return p


@pytest.mark.parametrize("cell,line_search,metric", [("fused_1d", None, "res_rms"), ("whole_run", "strong_wolfe", "res_rms"),
                                                     ("whole_run", "strong_wolfe", "energy"), ("padded_2d", None, "res_rms"),
                                                     ("mixture_1d", None, "energy")])
def test_keeper_keeps_what_select_names(cell, line_search, metric):
    make = _ls_fresh if line_search else (lambda: _cell_engine(cell))
    n_rec = LS_RECORDS
    a = make()
    _bind(a, keeper_kw=dict(metric=metric))
    a.lbfgs_monitor(True)
    a.lbfgs_run(n_rec * EVERY)
    recs, vals = _records(a), _column(a, metric)
    k, kept_all, _ = keeper.select(vals)
    print(f"   {cell} {line_search} {metric}: " + " ".join(f"{v:.6e}" for v in vals) + f" -> kept {k} of {kept_all}")
    assert len(recs) == n_rec and k is not None
    assert a.keeper_state() == dict(keeper.counters(n_rec, kept_all), stopped=False)
    assert _bytes(a.best_record()) == _bytes(recs[k])
    p_k = _judged_point_at(make, EVERY * (k + 1))
    np.testing.assert_array_equal(a.best_params(), p_k)
    a.restore_best()                                                                     # (under strong Wolfe: during a running search)
    np.testing.assert_array_equal(a.get_params(), p_k)
    st = a.lbfgs_read()
    assert st["n_iter"] == 0 and st["count"] == 0 and st["frozen"] == 0
    assert a.lbfgs_ls_read()["evals_total"] == 0 and a.lbfgs_ls_read()["phase"] == "none"
    np.testing.assert_array_equal(a.lbfgs_point(), p_k)
    a.close()


# ---- 4. patience freezes with code 4 -------------------------------------------------------------------------------------------------
PATIENCE = 2
# no line search at lr 1 on the whole-run problem, judged by the energy (which rises from the second record on) / the strong-Wolfe run
# judged by res_rms: the stop falls on a tick in the middle of a search (asserted on the reference)
STOP_CASES = {"plain_lr1": (None, "energy", 8), "strong_wolfe": ("strong_wolfe", "res_rms", 8)}


def _stop_make(line_search):
    if line_search:
        return _ls_fresh()
    flat, fun, factory, mse = lsb._whole_run("physics")
    eng = factory()
    eng.lbfgs_config(1.0, history=100, tolerance_grad=1e-30)
    return eng


@pytest.mark.parametrize("case", list(STOP_CASES))
def test_patience_freezes_with_code_4(case):
    line_search, metric, n_rec = STOP_CASES[case]
    make = lambda: _stop_make(line_search)
    u = make()                                                                           # the unstopped run
    _bind(u, keeper_kw=dict(metric=metric))
    u.lbfgs_monitor(True)
    u.lbfgs_run(n_rec * EVERY)
    vals, recs_u = _column(u, metric), _records(u)
    u.close()
    _, _, s = keeper.select(vals, patience=PATIENCE)
    print(f"   {case} {metric}: " + " ".join(f"{v:.6e}" for v in vals) + f" -> stop at record {s}")
    assert s is not None and 0 < s < n_rec - 1, (s, list(vals))                          # strictly inside the run
    if line_search:
        assert _ls_reference()[EVERY * (s + 1) - 1]["phase"] in ("bracket", "zoom")      # theta sits at a trial point when the stop fires
    p_s = _judged_point_at(make, EVERY * (s + 1))
    a = make()
    _bind(a, keeper_kw=dict(metric=metric, patience=PATIENCE))
    a.lbfgs_monitor(True)
    a.lbfgs_run(n_rec * EVERY)
    assert a.lbfgs_read()["frozen"] == FROZEN_KEEPER and gpe_pinn.Engine.LBFGS_FROZEN[FROZEN_KEEPER] == "keeper"
    np.testing.assert_array_equal(a.get_params(), p_s)
    np.testing.assert_array_equal(a.lbfgs_point(), p_s)
    assert a.stop_state()[0] is True and a.keeper_state()["stopped"] is True
    recs = _records(a)
    assert len(recs) == n_rec                                                            # records keep arriving
    for j in range(s + 1):
        assert _bytes(recs[j]) == _bytes(recs_u[j]), j
    for j in range(s + 1, n_rec):                                                        # ... of theta as it stands: the stopping record's
        assert _bytes(recs[j]) == _bytes(recs[s]), j
    before = _state(a)
    a.lbfgs_run(2 * EVERY)                                                               # 6 further ticks change no byte
    after = _state(a)
    np.testing.assert_array_equal(after[0], before[0])
    for x, y in zip(before[3], after[3]):
        np.testing.assert_array_equal(x, y)
    assert after[1]["frozen"] == FROZEN_KEEPER and after[1]["n_iter"] == before[1]["n_iter"] and after[2] == before[2]
    assert len(_records(a)) == n_rec + 2
    # re-arming: the keeper counts again from "nothing kept"; the stop and the freeze are cleared by what clears them after gpe_run
    # (reset_optimizer), and a new run then stops again at the same record
    (a.bind_mixture_keeper if a.cfg.mixture else a.bind_keeper)(metric=metric, patience=PATIENCE)
    assert a.keeper_state() == dict(seen=0, kept=0, since_best=0, stopped=False)
    flat = lsb._whole_run("physics")[0]
    a.set_params(flat)
    a.reset_optimizer(1e-3)
    assert a.lbfgs_read()["frozen"] == 0 and a.stop_state()[0] is False
    _bind(a, keeper_kw=dict(metric=metric, patience=PATIENCE))
    a.lbfgs_run(n_rec * EVERY)
    assert a.lbfgs_read()["frozen"] == FROZEN_KEEPER and a.keeper_state()["stopped"] is True
    np.testing.assert_array_equal(a.get_params(), p_s)
    a.close()


# ---- 5. off is off -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["never_called", "on_then_off"])
@pytest.mark.parametrize("line_search", [None, "strong_wolfe"])
def test_off_is_off(how, line_search):
    make = _ls_fresh if line_search else (lambda: _cell_engine("fused_2d"))
    a = make()
    _bind(a, keeper_kw=dict(metric="res_rms", patience=1))
    if how == "on_then_off":
        a.lbfgs_monitor(True)
        a.lbfgs_monitor(False)
    a.lbfgs_run(4 * EVERY)
    assert a.monitor_available() == 0 and a.keeper_state() == dict(seen=0, kept=0, since_best=0, stopped=False)
    c = make()
    c.lbfgs_run(4 * EVERY)
    _same_state(_state(a), _state(c), f"{how} {line_search}")
    a.close(); c.close()


# ---- 6. a freeze by tolerance_grad: records go on, of theta as it stands ---------------------------------------------------------------
def test_records_after_a_tolerance_grad_freeze():
    """The recipe of tests/test_gpu_lbfgs_ls.py::test_tolerance_grad_reached_at_an_accepted_point (injected gradients: the second tick
    accepts a nearly flat point and freezes with code 1), then ticks of lbfgs_run under the monitor."""
    cfg = dict(lr=1.0, history=3, tolerance_grad=1e-3, tolerance_change=1e-9)
    eng = ls_engine("P1153", cfg)
    g0 = np.random.default_rng(52).normal(0, 1, eng.n_params).astype(np.float32)
    base.inject(eng, g0, 4.0)
    trial = eng.get_params()
    base.inject(eng, (1e-4 * g0).astype(np.float32), 3.0)
    assert eng.lbfgs_read()["frozen"] == lr_.FROZEN_GRAD and eng.lbfgs_ls_read()["phase"] == "frozen"
    np.testing.assert_array_equal(eng.get_params(), trial)
    np.testing.assert_array_equal(eng.lbfgs_point(), trial)                              # frozen: theta as it stands
    want = _look(eng)
    _bind(eng, every=2)
    eng.lbfgs_monitor(True)
    hist = eng.lbfgs_history()
    eng.lbfgs_run(6)
    recs = _records(eng)
    assert len(recs) == 3
    for r in recs:
        assert _bytes(r) == _bytes(want)
    assert eng.lbfgs_read()["frozen"] == lr_.FROZEN_GRAD
    np.testing.assert_array_equal(eng.get_params(), trial)
    for x, y in zip(hist, eng.lbfgs_history()):
        np.testing.assert_array_equal(x, y)
    eng.close()


def test_records_after_a_nonfinite_freeze_at_a_trial():
    """Frozen code 2 is judged at theta: the recipe of tests/test_gpu_lbfgs_ls.py::test_nan_loss_at_a_trial_restores_the_low_end_and_freezes
    (its injected NaN loss at a zoom trial; nothing faults), then ticks of lbfgs_run under the monitor."""
    make, lr, seed = cases.TICK_CASES["quad_lr8"]
    cfg = dict(lr=lr, history=3, tolerance_grad=1e-30, tolerance_change=1e-9)
    eng = ls_engine("P1153", cfg)
    obj = make(eng.get_params(), seed)
    fun = lambda th: cases.injected(obj, th)
    for _ in range(cases.TICKS):
        loss, g = fun(eng.get_params())
        base.inject(eng, g, loss)
        if eng.lbfgs_ls_read()["phase"] == "zoom":
            break
    assert eng.lbfgs_ls_read()["phase"] == "zoom"
    assert (eng.lbfgs_point() != eng.get_params()).any()                                 # at a trial point
    base.inject(eng, fun(eng.get_params())[1], float("nan"))
    assert eng.lbfgs_read()["frozen"] == lr_.FROZEN_NONFINITE
    theta = eng.get_params()
    np.testing.assert_array_equal(eng.lbfgs_point(), theta)
    want = _look(eng)
    _bind(eng, every=2)
    eng.lbfgs_monitor(True)
    eng.lbfgs_run(4)
    recs = _records(eng)
    assert len(recs) == 2 and all(_bytes(r) == _bytes(want) for r in recs)
    np.testing.assert_array_equal(eng.get_params(), theta)
    eng.close()


# ---- 7. one rhythm across Adam and the tail ----------------------------------------------------------------------------------------------
def test_one_rhythm_across_adam_and_the_tail():
    def start():
        layers, path, kw, lr = CELLS["fused_2d"]
        eng = make_engine(layers, path, lr=1e-3, sched=capi.SCHED_CONST, **kw)
        return eng

    a = _bind(start(), every=5)
    a.run(7)
    assert a.monitor_available() == 1                                                    # count 5
    a.lbfgs_config(0.05, history=5, tolerance_grad=1e-30)
    a.lbfgs_monitor(True)
    a.lbfgs_run(2)
    assert a.monitor_available() == 1                                                    # count 9
    a.lbfgs_run(1)
    assert a.monitor_available() == 2                                                    # count 10
    a.lbfgs_run(5)
    recs = _records(a)
    assert len(recs) == 3                                                                # count 15
    assert [r["step"] for r in recs] == [5.0, 7.0, 7.0]                                  # the Adam step count, which L-BFGS does not advance
    b = start()
    b.run(7)
    b.lbfgs_config(0.05, history=5, tolerance_grad=1e-30)
    b.lbfgs_run(3)
    assert _bytes(_look(b)) == _bytes(recs[1])
    b.lbfgs_run(5)
    assert _bytes(_look(b)) == _bytes(recs[2])
    np.testing.assert_array_equal(a.get_params(), b.get_params())
    a.close(); b.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C
    layers, path = SHAPES["P1153"]
    eng = make_engine(layers, path)
    buf = np.zeros(eng.n_params, np.float32)
    vp = buf.ctypes.data_as(C.c_void_p)
    _raises(capi.GPE_ERR_STATE, eng.lbfgs_monitor, True)                                 # not configured
    _raises(capi.GPE_ERR_STATE, eng.lbfgs_point)
    eng.lbfgs_config(0.05, history=5, tolerance_grad=1e-30)
    assert eng.lib.gpe_lbfgs_monitor(eng._h, 2) == capi.GPE_ERR_INVALID
    assert eng.lib.gpe_lbfgs_monitor(eng._h, -1) == capi.GPE_ERR_INVALID
    assert eng.lib.gpe_lbfgs_point(eng._h, vp, eng.n_params + 1) == capi.GPE_ERR_INVALID
    assert eng.lib.gpe_lbfgs_point(eng._h, vp, eng.n_params - 1) == capi.GPE_ERR_INVALID
    assert eng.lib.gpe_lbfgs_point(eng._h, None, eng.n_params) == capi.GPE_ERR_INVALID
    assert eng.lib.gpe_lbfgs_point(eng._h, vp, eng.n_params) == capi.GPE_OK
    np.testing.assert_array_equal(buf, eng.get_params())
    # the flag survives lbfgs_config and gpe_lbfgs_line_search; with no monitor bound it does nothing
    eng.lbfgs_monitor(True)
    eng.lbfgs_config(0.05, history=7, tolerance_grad=1e-30)
    assert eng.lib.gpe_lbfgs_line_search(eng._h, 1, 1e-4, 0.9, 25) == capi.GPE_OK
    assert eng.lib.gpe_lbfgs_line_search(eng._h, 0, 1e-4, 0.9, 25) == capi.GPE_OK
    eng.lbfgs_run(2 * EVERY)
    c = make_engine(layers, path)
    c.lbfgs_config(0.05, history=7, tolerance_grad=1e-30)
    c.lbfgs_run(2 * EVERY)
    _same_state(_state(eng), _state(c), "flag on, nothing bound")
    _bind(eng)                                                                           # ... and it did survive: records now arrive
    eng.lbfgs_run(EVERY)
    assert eng.monitor_available() == 1
    c.lbfgs_run(EVERY)
    assert _bytes(_records(eng)[0]) == _bytes(_look(c))
    eng.close(); c.close()
