"""The strong-Wolfe line search of the device-resident L-BFGS (csrc/gpe_lbfgs_rules.h: ls_decide, ls_rearm; csrc/gpe_lbfgs.h: k_ls_dots,
k_ls_decide and the LS instantiations of k_lbfgs_dots / k_lbfgs_coef / k_lbfgs_apply) against the flat float64 reference tests/lbfgs_ls_ref.py, which
tests/test_lbfgs_ls_reference_cpu.py holds to torch.optim.LBFGS(line_search_fn="strong_wolfe").

Injection as in tests/test_gpu_lbfgs.py (its make_engine and inject): N = 256 points, gradient and loss written into exchange_grad between
step_backward() and lbfgs_update().  After every tick theta is read back, an analytic objective (tests/lbfgs_ls_cases.py) is evaluated there
in fp64, and its fp32 gradient and a loss float32 holds are injected; the reference is fed the same numbers, and at every accepted tick it
takes over the device's own fp32 state (start point, pairs, start gradient, direction).  Both sides therefore decide on identical inputs up
to the fp64 dot-product error (<= 4 P 2^-53 relative to sum |g_i d_i|), and a tick counts only if every comparison the reference made
kept a relative margin above 1e-6 -- which the CPU test asserts for these seeds on the reference alone; no tick is left out.

Per tick: phase, ls_iter, evaluation counts, low_pos, slots, counters and flags match EXACTLY; t of the next trial to 1e-9 relative; the trial
theta within 2 (u |theta| + u t |d|), u = 2^-24 (one rounding of an fp64 sum on each side); at accepted ticks the bounds of
tests/test_gpu_lbfgs.synced_iteration for the new direction (2 u |d| + eps_c sum_j |c_j b_j|, eps_c = 4 (P + 2 m) 2^-53), the new start
point EQUAL to the bits of the trial that was accepted, and g_prev equal to the bits of that trial's gradient.  None of these tolerances
was measured on the GPU.

Whole runs: invariants from the device's own records (exact), the loss trajectory against the fp64 reference driven by the fp64 oracle over
the leading ticks whose decision margins exceed 1e-3 (tolerance: the measured deviation times 4, profiles/lbfgs_ls/trajectory.txt), and
the engine against itself without the line search."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpe_pinn import GPEConfig, Engine, capi
from oracle import gpe_oracle as go
from tests import lbfgs_ls_cases as cases
from tests import lbfgs_ls_ref as ls_
from tests import lbfgs_ref as lr_
from tests import mse_ref
from tests import test_gpu_lbfgs as base

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N = cases.N
EXACT = ("phase", "ls_iter", "ls_evals", "evals_total", "low_pos", "insuf_progress", "slot_new", "accepted", "end_max_ls", "end_width",
         "end_curv", "stalled")


def ls_engine(shape, cfg, **ls):
    layers, path = base.SHAPES[shape]
    eng = base.make_engine(layers, path)
    eng.lbfgs_config(line_search="strong_wolfe", **cfg, **ls)
    return eng


class Pair:
    """An engine and the reference side by side: tick() evaluates `fun` at the device's theta, injects, ticks both and compares."""
    def __init__(self, eng, cfg, ls, what):
        self.eng, self.cfg, self.what = eng, cfg, what
        self.ref = ls_.LbfgsLsRef(eng.get_params(), ring_dtype=np.float32, exact_losses=True, **cfg, **ls)
        self.trials = {}                                  # step -> (theta bits, gradient bits) of the running search
        self.k = 0
        self.worst = 0.0

    def tick(self, fun, check_margin=False):
        eng, ref, what = self.eng, self.ref, f"{self.what} tick {self.k}"
        th = eng.get_params()
        t_now = ref.t if ref.state != ls_.IDLE else 0.0
        if not ref.lb.frozen:
            bound = 2 * (U * np.abs(ref.theta) + U * t_now * np.abs(ref.lb.d))
            err = np.abs(th.astype(np.float64) - ref.theta)
            self.worst = max(self.worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (what, float(err.max()), int(np.argmax(err - bound)))
        loss, g = fun(th)
        loss_in = base.inject(eng, g, loss)
        self.trials[t_now] = (th, np.asarray(g, np.float32))
        r = ref.tick(loss_in, np.asarray(g, np.float32))
        rec = eng.lbfgs_ls_read()
        self.k += 1
        if check_margin:
            assert r["min_margin"] > cases.MARGIN_CAP, (what, r["min_margin"])
        for f in EXACT:
            assert rec[f] == r[f], (what, f, rec[f], r[f])
        assert rec["bslots"] == r["bslot"][0] + 4 * r["bslot"][1], (what, rec["bslots"], r["bslot"])
        if not r["wrote"]:
            return rec, r
        for a, b in (("t", r["t_next"]), ("b0", r["b"][0]), ("b1", r["b"][1]), ("gtd0", r["gtd0"])):
            assert abs(rec[a] - b) <= 1e-9 * abs(b), (what, a, rec[a], b)
        dot_err = 4.0 * th.size * 2.0 ** -53 * r["gtd_scale"]       # a g.d that nearly cancels is known to the sum's error only
        for a, b in (("bgtd0", r["bgtd"][0]), ("bgtd1", r["bgtd"][1])):
            assert abs(rec[a] - b) <= 1e-9 * abs(b) + dot_err, (what, a, rec[a], b)
        assert (rec["bf0"], rec["bf1"], rec["f0"], rec["dnorm"]) == (r["bf"][0], r["bf"][1], r["f0"], r["dnorm"]), (what, rec, r["bf"], r["f0"])
        if r["phase"] == "accepted" or (r["phase"] == "frozen" and r["iteration"] is not None):
            self._accepted(r, what)
        return rec, r

    def _accepted(self, r, what):
        eng, ref, it = self.eng, self.ref, r["iteration"]
        lrec = eng.lbfgs_read()
        th0_bits, g_bits = self.trials[r["t_acc"]] if r["t_acc"] in self.trials else self.trials[0.0]
        assert lrec["n_iter"] == it["n_iter"] and lrec["count"] == it["count"] and lrec["frozen"] == it["frozen"], (what, lrec, it["n_iter"])
        assert lrec["loss"] == it["loss"], (what, lrec["loss"], it["loss"])
        if it["status"] == "frozen":
            np.testing.assert_array_equal(eng.get_params(), th0_bits, err_msg=what)      # left at the accepted point
            return
        assert lrec["t"] == it["t"] and lrec["pushed"] == it["pushed"] and lrec["skipped"] == (it["status"] == "skipped"), (what, lrec, it["t"])
        assert lrec["grad_max"] == it["grad_max"] and abs(lrec["gtd"] - it["gtd"]) <= 1e-9 * abs(it["gtd"]), (what, lrec["gtd"], it["gtd"])
        S, Y, gp, d = eng.lbfgs_history()
        np.testing.assert_array_equal(gp, g_bits, err_msg=what)                          # the STORED gradient of the accepted point
        P, m = d.size, self.cfg["history"]
        bound = 2 * U * np.abs(it["d"]) + 4.0 * (P + 2 * m) * 2.0 ** -53 * it["absum"]
        err = np.abs(d.astype(np.float64) - it["d"])
        assert (err <= bound).all(), (what, "direction", float(err.max()))
        ref.resync(th0_bits, S, Y, gp, d)
        self.trials = {0.0: (th0_bits, g_bits)}
        if it["status"] == "skipped":
            np.testing.assert_array_equal(eng.get_params(), th0_bits, err_msg=what)


@pytest.mark.parametrize("history", [3, 10])
@pytest.mark.parametrize("case", list(cases.TICK_CASES))
@pytest.mark.parametrize("shape", list(base.SHAPES))
def test_tick_by_tick_against_the_reference(shape, case, history):
    make, lr, seed = cases.TICK_CASES[case]
    cfg = dict(lr=lr, history=history, tolerance_grad=1e-30, tolerance_change=1e-9)
    eng = ls_engine(shape, cfg)
    np.testing.assert_array_equal(eng.get_params(), cases.start_params(eng.n_params))   # the start the CPU test asserted the margins for
    obj = make(eng.get_params(), seed)
    pair = Pair(eng, cfg, {}, f"{shape} {case} m={history}")
    phases = []
    for _ in range(cases.TICKS):
        rec, r = pair.tick(lambda th: cases.injected(obj, th), check_margin=True)
        phases.append(r["phase"])
    print(f"[{shape} {case} m={history}] worst trial err/bound {pair.worst:.3f}; {phases}")
    assert len(phases) >= 12 and phases.count("accepted") >= 2 and "frozen" not in phases
    assert ("bracket" in phases) if case == "quad_lr0.01" else True
    assert ("zoom" in phases) if case == "quad_lr8" else True
    eng.close()


def _cell(name):
    phi, dphi, lr, kw, end = cases.END_CELLS[name]
    kw = dict(kw)
    cfg = dict(lr=lr, history=3, tolerance_grad=1e-30, tolerance_change=kw.pop("tolerance_change", 1e-9))
    eng = ls_engine("P1153", cfg, **kw)
    obj = cases.LineProfile(eng.get_params(), phi, dphi)
    pair = Pair(eng, cfg, kw, name)
    fun = lambda th: cases.injected(obj, th)
    pair.tick(fun)                                        # the evaluation at the start: direction and first trial
    thetas, steps = [], []
    for _ in range(70):
        thetas.append(eng.get_params()); steps.append(pair.ref.t)
        rec, r = pair.tick(fun)
        if r["phase"] in ("accepted", "frozen"):
            break
    assert r["phase"] == "accepted" and rec[end] == 1 and rec["accepted"] == 1, (name, rec)
    return eng, pair, rec, r, thetas, steps


def test_end_max_ls_fallback():
    eng, pair, rec, r, thetas, steps = _cell("max_ls")
    assert len(steps) == 4 and r["ls_iter"] == 0 and rec["end_curv"] == 0 and rec["end_width"] == 0
    assert r["t_acc"] == steps[-1]                        # the falling profile: the far end of the fallback bracket [0, t]
    eng.close()


def test_end_bracket_width_break():
    eng, pair, rec, r, thetas, steps = _cell("width")
    assert rec["end_max_ls"] == 0 and rec["end_curv"] == 0
    eng.close()


def test_an_accepted_point_that_is_not_the_last_evaluated():
    eng, pair, rec, r, thetas, steps = _cell("not_last")
    k = steps.index(r["t_acc"])
    assert k < len(steps) - 1, (steps, r["t_acc"])
    # the new start point is the EARLIER trial's bits (Pair._accepted has held g_prev to that trial's gradient bits): read it through a
    # reset, which ends the new search by putting theta back to its start point
    eng.reset_optimizer(1e-3)
    np.testing.assert_array_equal(eng.get_params(), thetas[k])
    eng.close()


def test_stalled_search_leaves_theta_and_counts():
    cfg = dict(lr=1.0, history=3, tolerance_grad=1e-30, tolerance_change=1e-9)
    eng = ls_engine("P1153", cfg, max_ls=4)
    pair = Pair(eng, cfg, dict(max_ls=4), "stalled")
    th0 = eng.get_params()
    g0 = np.random.default_rng(51).normal(0, 1, eng.n_params).astype(np.float32)
    pair.tick(lambda th: (4.0, g0))
    for k in range(8):                                    # the loss rises wherever it is tried: the bracket closes on t = 0
        rec, r = pair.tick(lambda th: (5.0 + k, g0))
        if r["phase"] == "accepted":
            break
    assert rec["stalled"] == 1 and r["t_acc"] == 0.0 and eng.lbfgs_read()["pushed"] == 0
    eng.reset_optimizer(1e-3)                             # ends the new search: theta back at its start point, the unchanged theta0
    np.testing.assert_array_equal(eng.get_params(), th0)
    eng.close()


def test_nan_loss_at_a_trial_restores_the_low_end_and_freezes():
    make, lr, seed = cases.TICK_CASES["quad_lr8"]
    cfg = dict(lr=lr, history=3, tolerance_grad=1e-30, tolerance_change=1e-9)
    eng = ls_engine("P1153", cfg)
    obj = make(eng.get_params(), seed)
    pair = Pair(eng, cfg, {}, "nan trial")
    fun = lambda th: cases.injected(obj, th)
    for _ in range(cases.TICKS):
        rec, r = pair.tick(fun)
        if r["phase"] == "zoom":
            break
    assert r["phase"] == "zoom"
    t_low = pair.ref.b[pair.ref.low_pos]
    thetas = {t: bits for t, (bits, _) in pair.trials.items()}      # the device's theta at every step this search has evaluated
    rec, r = pair.tick(lambda th: (float("nan"), fun(th)[1]))
    assert r["phase"] == "frozen" and rec["phase"] == "frozen" and eng.lbfgs_read()["frozen"] == lr_.FROZEN_NONFINITE
    np.testing.assert_array_equal(eng.get_params(), thetas[t_low])
    hist, before = eng.lbfgs_history(), eng.lbfgs_ls_read()
    for _ in range(2):                                    # later ticks write nothing
        base.inject(eng, fun(eng.get_params())[1], 1.0)
    np.testing.assert_array_equal(eng.get_params(), thetas[t_low])
    assert eng.lbfgs_ls_read() == before
    for a, b in zip(hist, eng.lbfgs_history()):
        np.testing.assert_array_equal(a, b)
    eng.close()


def test_tolerance_grad_reached_at_an_accepted_point():
    cfg = dict(lr=1.0, history=3, tolerance_grad=1e-3, tolerance_change=1e-9)
    eng = ls_engine("P1153", cfg)
    pair = Pair(eng, cfg, {}, "tolerance_grad")
    g0 = np.random.default_rng(52).normal(0, 1, eng.n_params).astype(np.float32)
    pair.tick(lambda th: (4.0, g0))
    trial = eng.get_params()
    rec, r = pair.tick(lambda th: (3.0, (1e-4 * g0).astype(np.float32)))      # lower, nearly flat: the curvature test accepts it
    assert r["phase"] == "frozen" and rec["phase"] == "frozen" and rec["end_curv"] == 1
    assert eng.lbfgs_read()["frozen"] == lr_.FROZEN_GRAD
    np.testing.assert_array_equal(eng.get_params(), trial)
    eng.close()


def test_line_search_off_is_the_machine_as_it_was():
    layers, path = base.SHAPES["P12737"]
    thetas = []
    for call in (False, True):
        eng = base.make_engine(layers, path)
        eng.lbfgs_config(lr=0.1, history=4, tolerance_grad=1e-30)
        if call:
            assert eng.lib.gpe_lbfgs_line_search(eng._h, 1, 1e-4, 0.9, 25) == capi.GPE_OK      # on (allocates), and off again
            assert eng.lib.gpe_lbfgs_line_search(eng._h, 0, 1e-4, 0.9, 25) == capi.GPE_OK
        q = base.Quadratic(eng.get_params(), 13)
        for k in range(10):
            base.inject(eng, q.grad(eng.get_params()), 1.0 + 1.0 / (k + 1))
        thetas.append((eng.get_params(), eng.lbfgs_read(), eng.lbfgs_history()))
        eng.close()
    np.testing.assert_array_equal(thetas[0][0], thetas[1][0])
    assert thetas[0][1] == thetas[1][1]
    for a, b in zip(thetas[0][2], thetas[1][2]):
        np.testing.assert_array_equal(a, b)


def test_bit_repeatability():
    out = []
    make, lr, seed = cases.TICK_CASES["quad_lr8"]
    for _ in range(2):
        eng = ls_engine("P12737", dict(lr=lr, history=4, tolerance_grad=1e-30))
        obj = make(eng.get_params(), seed)
        recs = []
        for k in range(30):
            loss, g = cases.injected(obj, eng.get_params())
            base.inject(eng, g, loss)
            recs.append((eng.lbfgs_ls_read(), eng.lbfgs_read()))
        out.append((eng.get_params(), recs))
        eng.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


def test_resets_end_a_running_search():
    make, lr, seed = cases.TICK_CASES["quad_lr8"]
    cfg = dict(lr=lr, history=3, tolerance_grad=1e-30)
    eng = ls_engine("P1153", cfg)
    obj = make(eng.get_params(), seed)
    start = eng.get_params()
    base.inject(eng, *reversed(cases.injected(obj, start)))
    assert (eng.get_params() != start).any() and eng.lbfgs_ls_read()["phase"] == "accepted"      # at the first trial of the first search
    eng.reset_optimizer(1e-3)
    np.testing.assert_array_equal(eng.get_params(), start)
    st = eng.lbfgs_ls_read()
    assert st["phase"] == "none" and st["evals_total"] == 0 and eng.lbfgs_read()["n_iter"] == 0
    base.inject(eng, *reversed(cases.injected(obj, start)))
    other = (start * 0.5).astype(np.float32)
    eng.set_params(other)
    np.testing.assert_array_equal(eng.get_params(), other)
    assert eng.lbfgs_ls_read()["evals_total"] == 0
    eng.close()


def test_refusals():
    layers, path = base.SHAPES["P1153"]
    eng = base.make_engine(layers, path)
    ls = lambda *a: eng.lib.gpe_lbfgs_line_search(eng._h, *a)
    out = (C.c_double * len(Engine.LBFGS_LS_FIELDS))()
    assert ls(1, 1e-4, 0.9, 25) == capi.GPE_ERR_STATE and eng.lib.gpe_lbfgs_ls_read(eng._h, out) == capi.GPE_ERR_STATE      # not configured
    eng.lbfgs_config(0.1, history=3)
    for bad in ((2, 1e-4, 0.9, 25), (-1, 1e-4, 0.9, 25), (1, float("nan"), 0.9, 25), (1, 1e-4, float("inf"), 25), (1, 0.0, 0.9, 25),
                (1, 0.9, 0.9, 25), (1, 0.95, 0.9, 25), (1, 1e-4, 1.0, 25), (1, 1e-4, 0.9, 0), (1, 1e-4, 0.9, 65)):
        assert ls(*bad) == capi.GPE_ERR_INVALID, bad
    assert ls(1, 1e-4, 0.9, 64) == capi.GPE_OK and ls(1, 1e-4, 0.9, 1) == capi.GPE_OK and ls(0, 1e-4, 0.9, 25) == capi.GPE_OK
    with pytest.raises(ValueError):
        eng.lbfgs_config(0.1, history=3, line_search="backtracking")
    eng.lbfgs_config(0.1, history=3, line_search="strong_wolfe")
    with pytest.raises(base.GPEError, match="without step_backward"):
        eng.lbfgs_update()
    eng.bind_sampler([-3.0], [3.0], [N], every=2, seed=1)                     # the refusals of update / run stand
    with pytest.raises(base.GPEError, match="sampler"):
        eng.lbfgs_run(1)
    eng.close()


# ---- whole runs ---------------------------------------------------------------------------------------------------------------------
def _whole_run(kind):
    layers = [1, 32, 32, 1]
    x = np.linspace(-4, 4, N).reshape(-1, 1)
    if kind == "mse":
        target = (np.pi ** -0.25 * np.exp(-0.5 * x ** 2))
        flat = np.random.default_rng(21).normal(0, 0.4, go.param_count(layers)).astype(np.float32)
        pb = go.Problem(layers=layers, w_bc=0.0)
        fun = lambda th: mse_ref.mse_loss_and_grad(pb, th, x, target)

        def factory():
            e = Engine(GPEConfig(layers=layers, w_bc=0.0, lr=1e-3, sched=capi.SCHED_CONST))
            e.set_params(flat)
            e.bind_points(torch.as_tensor(x.astype(np.float32), device="cuda"))
            e.bind_target(torch.as_tensor(target.astype(np.float32), device="cuda"))
            return e
    else:
        kw = dict(layers=layers, gamma=1.0, p=3, dx=8.0 / N, w_bc=0.0)
        flat = np.random.default_rng(22).normal(0, 0.4, go.param_count(layers)).astype(np.float32)
        pb = go.Problem(**kw)

        def fun(th):
            sc, g, _ = go.full_loss_and_grad(pb, th, x)
            return sc["loss"], g

        def factory():
            e = Engine(GPEConfig(**kw))
            e.set_params(flat)
            e.bind_points(torch.as_tensor(x.astype(np.float32), device="cuda"))
            return e
    return flat, fun, factory, kind == "mse"


C1, C2, N_EVAL = 1e-4, 0.9, 40
# The issue fixes lr = 1 for the comparison against the engine without the line search and leaves the lr of the other whole-run checks
# open.  At lr = 1 the fp64 reference ALONE (no device involved) has a single leading tick with margins above 1e-3 on the pre-training
# loss: its first trial is the step lr / |g|_1, along which the loss falls by 9.6e-5 of itself, so tick 1's sufficient-decrease comparison
# has a relative margin of 9.6e-5.  LR_TRAJ is the smallest power of two at which the reference alone has at least 10 leading ticks on BOTH
# losses (20 on the pre-training loss, 23 on the physics loss; lr = 1: 1 and 14); it was chosen from the reference's margins on the CPU,
# before any device run at it.  At 2 the runs also pass through the bracket and zoom phases, which at lr = 1 they hardly do.
LR_VS_PLAIN, LR_TRAJ = 1.0, 2.0
_RUNS = {}


def _run(kind, lr):
    """One run per kind and lr, shared by the tests below and left unchanged: the fp64 reference on the fp64 oracle, the device with the
    line search (its record after every tick) and the device without it, from the same start at the same lr."""
    if (kind, lr) in _RUNS:
        return _RUNS[kind, lr]
    flat, fun, factory, mse = _whole_run(kind)
    outs = ls_.run_flat(ls_.LbfgsLsRef(flat, lr, 100), fun, N_EVAL) if lr == LR_TRAJ else None
    eng = factory()
    eng.lbfgs_config(lr, history=100, line_search="strong_wolfe", c1=C1, c2=C2)
    got = [eng.lbfgs_ls_read()]
    for _ in range(N_EVAL):
        eng.lbfgs_run(1, mse=mse)
        got.append(eng.lbfgs_ls_read())
    eng.close()
    end_plain = None
    if lr == LR_VS_PLAIN:
        plain = factory()
        plain.lbfgs_config(lr, history=100)
        plain.lbfgs_run(N_EVAL, mse=mse)
        end_plain = plain.lbfgs_read()["loss"]
        plain.close()
    _RUNS[kind, lr] = (outs, got, end_plain)
    return _RUNS[kind, lr]


@pytest.mark.parametrize("lr", [LR_VS_PLAIN, LR_TRAJ])
@pytest.mark.parametrize("kind", ["physics", "mse"])
def test_whole_run_invariants_from_the_devices_own_records(kind, lr):
    """Exact, from gpe_lbfgs_ls_read alone: the search that ended in a tick started at the previous record's (f0, gtd0) and accepted the
    point the new record keeps in bracket end 1 (step, loss, g.d)."""
    outs, got, _ = _run(kind, lr)
    accepted = []
    for k, (prev, rec) in enumerate(zip(got, got[1:])):
        if rec["accepted"] > prev["accepted"]:
            t_acc, f_acc, gtd_acc = rec["b1"], rec["bf1"], rec["bgtd1"]
            assert f_acc <= prev["f0"] + C1 * t_acc * prev["gtd0"], (k, f_acc, prev["f0"], t_acc, prev["gtd0"])
            if rec["end_curv"] > prev["end_curv"]:
                assert abs(gtd_acc) <= -C2 * prev["gtd0"], (k, gtd_acc, prev["gtd0"])
            accepted.append(f_acc)
    assert len(accepted) >= 5 and all(b <= a for a, b in zip(accepted, accepted[1:])), accepted
    assert got[-1]["evals_total"] == N_EVAL


@pytest.mark.parametrize("kind", ["physics", "mse"])
def test_whole_run_trajectory_against_the_fp64_reference(kind):
    """The accepted loss (f0 of the running search) tick by tick, and the phase of every tick, over the leading ticks whose decision
    margins in the fp64 reference exceed 1e-3; their number is computed here on the CPU and must be at least 10 (lr: see LR_TRAJ)."""
    outs, got, _ = _run(kind, LR_TRAJ)
    got = got[1:]
    lead = next((k for k, o in enumerate(outs) if o["min_margin"] <= 1e-3), N_EVAL)
    assert lead >= 10, (lead, [o["min_margin"] for o in outs[:10]])
    rel = max(abs(got[k]["f0"] - outs[k]["f0"]) / abs(outs[k]["f0"]) for k in range(lead))
    phases = [g["phase"] for g in got[:lead]]
    print(f"[whole run {kind} lr {LR_TRAJ}] leading ticks {lead}; worst relative deviation of the accepted loss {rel:.3e}; losses "
          f"{outs[0]['f0']:.4g} -> {outs[lead - 1]['f0']:.4g}; phases {phases}")
    assert phases == [o["phase"] for o in outs[:lead]]
    assert rel <= TRAJ_TOL[kind], (rel, TRAJ_TOL[kind])


@pytest.mark.parametrize("kind", ["physics", "mse"])
def test_whole_run_against_the_engine_without_the_line_search(kind):
    outs, got, end_plain = _run(kind, LR_VS_PLAIN)
    end_ls = got[-1]["f0"]
    print(f"[whole run {kind} lr {LR_VS_PLAIN}] last accepted loss after {N_EVAL} evaluations with the line search {end_ls:.6e} "
          f"({got[-1]['accepted']} searches); loss of the 40th iteration without it {end_plain:.6e}")
    if kind == "physics":
        assert end_ls < end_plain, (end_ls, end_plain)      # measured 2.689362e-01 against 2.709398e-01
    else:
        # "Lower" does NOT hold at this start, and the start is not tuned: every one of the 39 searches accepts its first trial t = lr = 1
        # (sufficient decrease and curvature hold there), so the run with the line search IS the run without it -- measured
        # 1.924827e-05 on both, 1.916e-05 on both in the fp64 reference.  What holds, and is asserted: not higher.
        assert end_ls <= end_plain, (end_ls, end_plain)


# measured once against the fp64 trajectory (profiles/lbfgs_ls/trajectory.txt), times 4 for box-to-box and seed spread
TRAJ_TOL = {"physics": 4 * 5.783e-05,     # measured 5.783e-05 over 23 leading ticks (losses 2059 -> 0.36)
            "mse": 4 * 4.126e-05}         # measured 4.126e-05 over 20 leading ticks (losses 7.5 -> 1.8e-4)
