#!/usr/bin/env python3
"""Cost of one monitor tick of an L-BFGS run (Engine.lbfgs_monitor): the view, the monitor chain, the unview and the repack the next
evaluation does anyway -- next to the cost of one record in an Adam run of the same shape.

[2,64,64,64,1], 65 536 training points, 3 001 held-out points, every = 10.  The same lbfgs_run with the flag off and on (monitor and keeper
bound either way), HIP events on the engine's stream around the whole run, alternating, median [min .. max] of --reps; then gpe_run without and with
the monitor and keeper.  The difference of the medians times `every` is the cost of one record.

usage: python tools/lbfgs_monitor_time.py [--ticks 300 --reps 9 --out profiles/lbfgs_monitor/tick_time.txt]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import gpe_pinn
from gpe_pinn import capi

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=65536)
ap.add_argument("--held-out", type=int, default=3001)
ap.add_argument("--every", type=int, default=10)
ap.add_argument("--ticks", type=int, default=300)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default="")
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


import bench
layers = [2, 64, 64, 64, 1]
n = int(round(a.points ** 0.5))
ax = np.linspace(-8.0, 8.0, n, dtype=np.float32)
X = np.stack([m.ravel() for m in np.meshgrid(ax, ax, indexing="ij")], axis=1)
dv = float(ax[1] - ax[0]) ** 2
xm = torch.as_tensor(np.random.default_rng(3).uniform(-8, 8, (a.held_out, 2)).astype(np.float32), device="cuda")
dvm = 256.0 / a.held_out
flat = bench.reference_init(layers, seed=0)


def engine():
    eng = gpe_pinn.Engine(gpe_pinn.GPEConfig(layers=layers, gamma=500.0, dx=dv, w_bc=0.0, lr=1e-4, sched=capi.SCHED_CONST, history_capacity=8))
    eng.set_params(flat)
    eng.bind_points(torch.as_tensor(X, device="cuda"))
    return eng


def timed(fn, n_steps):
    """device time per step in microseconds, HIP events around the whole run"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); fn(n_steps); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n_steps


say(f"device {torch.cuda.get_device_name(0)}   {layers}, {X.shape[0]} training points, {a.held_out} held-out points, every = {a.every}, "
    f"{a.ticks} steps per run, median of {a.reps} runs each, alternating")
med = lambda v: float(np.median(v))
results = {}
for ls in (None, "strong_wolfe"):
    eng = engine()
    eng.bind_monitor(xm, every=a.every, dv=dvm)
    eng.bind_keeper("res_rms")
    off, on = [], []
    for r in range(a.reps + 1):                     # (run 0 warms up: code objects, allocations)
        for flag, dst in ((False, off), (True, on)):
            eng.set_params(flat)                    # the same run every time: resets the L-BFGS state
            eng.lbfgs_config(0.05, history=10, tolerance_grad=1e-30, line_search=ls)
            eng.lbfgs_monitor(flag)
            t = timed(eng.lbfgs_run, a.ticks)
            if r:
                dst.append(t)
    st = eng.lbfgs_read()
    per_rec = (med(on) - med(off)) * a.every
    results[ls] = per_rec
    say(f"lbfgs_run, line search {ls}: {med(off):.2f} [{min(off):.2f} .. {max(off):.2f}] us/tick flag off, {med(on):.2f} [{min(on):.2f} .. {max(on):.2f}] us/tick flag on "
        f"-> {per_rec:.1f} us per monitor tick "
        f"(view + chain + keeper + unview + the repack; {eng.monitor_available()} records in the last run, frozen {st['frozen']})")
    eng.close()

eng = engine()
off, on = [], []
for r in range(a.reps + 1):
    for flag, dst in ((False, off), (True, on)):
        eng.set_params(flat)
        eng.reset_optimizer(1e-4)
        if flag:
            eng.bind_monitor(xm, every=a.every, dv=dvm)
            eng.bind_keeper("res_rms")
        else:
            eng.clear_monitor()
        t = timed(eng.run, a.ticks)
        if r:
            dst.append(t)
per_rec_adam = (med(on) - med(off)) * a.every
say(f"gpe_run (Adam), same shape: {med(off):.2f} us/step without monitor, {med(on):.2f} us/step with monitor and keeper -> {per_rec_adam:.1f} us per record")
say(f"one L-BFGS monitor tick costs {results[None] / per_rec_adam:.2f}x (no line search) / {results['strong_wolfe'] / per_rec_adam:.2f}x (strong Wolfe) "
    f"an Adam record")
eng.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
