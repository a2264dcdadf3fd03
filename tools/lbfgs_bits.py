#!/usr/bin/env python3
"""L-BFGS BITS: one sha256 per cell over everything a run of the device-resident L-BFGS leaves behind -- the raw fp32 bytes of
get_params(), lbfgs_point() and lbfgs_history(), the doubles of lbfgs_read() and lbfgs_ls_read() after EVERY tick -- and, in the monitor
cells, the monitor ring and best_record().  Fixed seeds, injected gradients and losses (tests/test_gpu_lbfgs.inject, the objectives of
tests/lbfgs_ls_cases.py), shapes P1153 (no multiple of 4, 64, 256 or 512: every tail loop runs) and P33537 (66 workgroups in the dots
kernels) at N = 256.  Run it once per library build (GPE_HIP_LIB=...) and diff the outputs: a change of the L-BFGS code that is a
refactor reproduces every hash.   usage: tools/lbfgs_bits.py > bits.txt"""
import hashlib, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPE_GEN_MIN_CHUNK", "256")
from tests import lbfgs_ls_cases as cases
from tests import test_gpu_lbfgs as base
from tests import test_gpu_lbfgs_monitor as mon

SHAPES = ("P1153", "P33537")


def doubles(e, rec):
    """a record of lbfgs_read / lbfgs_ls_read as the doubles the library wrote (the phase's name back to its index)"""
    return np.array([e.LBFGS_LS_PHASES.index(v) if isinstance(v, str) else v for v in rec.values()], np.float64).tobytes()


class Cell:
    """an engine, a hash that takes every read after every tick, and the injection"""
    def __init__(self, shape, line_search, **cfg):
        layers, path = base.SHAPES[shape]
        self.eng = base.make_engine(layers, path)
        self.eng.lbfgs_config(line_search=line_search, **dict(dict(tolerance_grad=1e-30), **cfg))
        self.h, self.k = hashlib.sha256(), 0
        self.g = None

    def look(self, full=False):
        e = self.eng
        self.h.update(e.get_params().tobytes())
        self.h.update(doubles(e, e.lbfgs_read()) + doubles(e, e.lbfgs_ls_read()))
        if full:
            self.h.update(e.lbfgs_point().tobytes())
            for a in e.lbfgs_history():
                self.h.update(a.tobytes())

    def tick(self, obj, loss=None, scale=None, same_gradient=False):
        """evaluate obj at theta and inject; loss: in its place; scale: times the gradient; same_gradient: the previous tick's again"""
        f, g = cases.injected(obj, self.eng.get_params())
        if same_gradient:
            g = self.g
        self.g = g
        base.inject(self.eng, g if scale is None else (g * np.float32(scale)), f if loss is None else loss)
        self.k += 1
        self.look(full=self.k % 4 == 0)

    def done(self, name):
        self.look(full=True)
        r, l = self.eng.lbfgs_read(), self.eng.lbfgs_ls_read()
        print(f"{name}: {self.h.hexdigest()[:16]}   ticks {self.k} n_iter {r['n_iter']} pairs {r['count']} head {r['head']} frozen {r['frozen']} "
              f"skipped {r['skipped']} phase {l['phase']} accepted {l['accepted']} stalled {l['stalled']}", flush=True)
        self.eng.close()


def objective(cell, case):
    make, lr, seed = cases.TICK_CASES[case]
    return make(cell.eng.get_params(), seed), lr


def sequence(shape, case, history, ls):
    """>= 8 accepted iterations at history 3 (the ring wraps) and a pair that is not pushed: without a line search the same gradient twice
    (y = 0); with it a loss that rises wherever it is tried, so the search closes on t = 0 (stalled: s = 0)"""
    lr = cases.TICK_CASES[case][1]
    c = Cell(shape, "strong_wolfe" if ls else None, lr=lr, history=history)
    obj, _ = objective(c, case)
    if not ls:
        for k in range(12):
            c.tick(obj, same_gradient=k == 7)
    else:
        for _ in range(30):
            c.tick(obj)
        stalled, f = c.eng.lbfgs_ls_read()["stalled"], cases.injected(obj, c.eng.get_params())[0]
        for k in range(40):
            if c.eng.lbfgs_ls_read()["stalled"] > stalled:
                break
            c.tick(obj, loss=f + 1.0 + k, same_gradient=k > 0)
        for _ in range(10):
            c.tick(obj)
    c.done(f"sequence {shape} {case} history {history} {'strong_wolfe' if ls else 'plain'}")


def endings(shape, ls):
    name = "strong_wolfe" if ls else "plain"
    search = "strong_wolfe" if ls else None
    # tolerance_grad: a gradient of 1e-12 times the objective's, at a lower loss (under strong Wolfe: accepted, then frozen), 3 ticks on
    c = Cell(shape, search, lr=0.01, history=3, tolerance_grad=1e-7)
    obj, _ = objective(c, "quad_lr0.01")
    for _ in range(5):
        c.tick(obj)
    for _ in range(4):
        c.tick(obj, loss=1e-3, scale=1e-12)
    c.done(f"ending tolerance_grad {shape} {name}")
    c = Cell(shape, search, lr=0.01, history=3, stop_loss=1e-2)
    obj, _ = objective(c, "quad_lr0.01")
    for _ in range(5):
        c.tick(obj)
    for _ in range(4):
        c.tick(obj, loss=1e-3, scale=1e-6)
    c.done(f"ending stop_loss {shape} {name}")
    c = Cell(shape, search, lr=0.01, history=3, tolerance_change=1e30)       # every iteration is a g.d skip
    obj, _ = objective(c, "quad_lr0.01")
    for _ in range(4):
        c.tick(obj)
    c.done(f"ending gtd_skip {shape} {name}")
    if ls:                                                                   # a NaN trial in zoom, and one in the bracket phase
        for phase, case in (("zoom", "quad_lr8"), ("bracket", "quad_lr0.01")):
            c = Cell(shape, search, lr=cases.TICK_CASES[case][1], history=3)
            obj, _ = objective(c, case)
            for _ in range(20):
                c.tick(obj)
                if c.eng.lbfgs_ls_read()["phase"] == phase:
                    break
            assert c.eng.lbfgs_ls_read()["phase"] == phase, phase
            c.tick(obj, loss=float("nan"))
            c.tick(obj)
            c.done(f"ending nan_in_{phase} {shape} {name}")


def resets(shape, ls):
    """set_params, and lbfgs_config with a new history (same line search: through the C entry points, as Engine.lbfgs_config calls them),
    each in the middle of a run -- under strong Wolfe in the middle of a search -- then five more ticks"""
    name = "strong_wolfe" if ls else "plain"
    for what in ("set_params", "new_history"):
        c = Cell(shape, "strong_wolfe" if ls else None, lr=8.0, history=3)
        obj, _ = objective(c, "quad_lr8")
        for _ in range(20):
            c.tick(obj)
            if c.k >= 6 and (not ls or c.eng.lbfgs_ls_read()["phase"] in ("bracket", "zoom")):
                break
        if what == "set_params":
            c.eng.set_params(cases.start_params(c.eng.n_params, seed=6))
        else:
            c.eng.lbfgs_config(8.0, history=7, tolerance_grad=1e-30, line_search="strong_wolfe" if ls else None)
        c.look(full=True)
        for _ in range(5):
            c.tick(obj)
        c.done(f"reset {what} {shape} {name}")


def monitored(line_search, metric, patience, buffers_only=False):
    """tests/test_gpu_lbfgs_monitor.py's stopping runs: 24 ticks, a record every third; patience 2 fires inside the run (frozen code 4).
    buffers_only: the line search was on once and is off: its buffers exist, the keeper's freeze writes its record too"""
    e = mon._stop_make(line_search)
    if buffers_only:
        e.lbfgs_config(1.0, history=100, tolerance_grad=1e-30, line_search="strong_wolfe")
        e.lbfgs_config(1.0, history=100, tolerance_grad=1e-30)
    mon._bind(e, keeper_kw=dict(metric=metric, patience=patience))
    e.lbfgs_monitor(True)
    e.lbfgs_run(24)
    h = hashlib.sha256()
    for a in (e.get_params(), e.lbfgs_point(), *e.lbfgs_history()):
        h.update(a.tobytes())
    h.update(doubles(e, e.lbfgs_read()) + doubles(e, e.lbfgs_ls_read()))
    for rec in (e.best_record(), *mon._records(e)):
        h.update(mon._bytes(rec))
    print(f"monitor {line_search or ('plain, line-search buffers held' if buffers_only else 'plain')} {metric} patience {patience}: "
          f"{h.hexdigest()[:16]}   frozen {e.lbfgs_read()['frozen']} ls phase {e.lbfgs_ls_read()['phase']} {e.keeper_state()}", flush=True)
    e.close()


for shape in SHAPES:
    for history in (3, 100):
        for ls in (False, True):
            for case in cases.TICK_CASES:
                sequence(shape, case, history, ls)
    for ls in (False, True):
        endings(shape, ls)
        resets(shape, ls)
for line_search, metric, _ in mon.STOP_CASES.values():
    for patience in (2, 0):
        monitored(line_search, metric, patience)
monitored(None, "energy", 2, buffers_only=True)
