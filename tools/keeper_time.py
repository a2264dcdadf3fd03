#!/usr/bin/env python3
"""Cost of the keeper (Engine.bind_keeper): gpe_run with a monitor, with and without the keeper on the same engine, interleaved.

(1) 1 048 576 points, monitor of the training grid's size at every = 100: step time (wall, run + synchronise).
(2) 3 969 points under graph replay, 16 384-point monitor at every = 100: host enqueue and total time per step.
The yardstick is the same run without the keeper on the same build: the keeper adds launches beside the step and changes no kernel of
it (tools/slab_sum_bits.py gives the same hashes with and without this feature).  Median of --reps runs each, A/B/A/B on one box.

usage: python tools/keeper_time.py [--points 1048576 --steps 300 --reps 9 --out profiles/keeper/keeper_time.txt]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import gpe_pinn
from gpe_pinn import capi

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=1 << 20)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--small-steps", type=int, default=2000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default="")
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def grid2d(n_points, half=8.0):
    n = int(round(n_points ** 0.5))
    ax = np.linspace(-half, half, n, dtype=np.float32)
    X = np.stack([m.ravel() for m in np.meshgrid(ax, ax, indexing="ij")], axis=1)
    return X, float(ax[1] - ax[0]) ** 2


def engine(layers, X, dv):
    import bench
    cfg = gpe_pinn.GPEConfig(layers=layers, gamma=500.0, dx=dv, w_bc=0.0, lr=1e-4, sched=capi.SCHED_CONST, history_capacity=8)
    eng = gpe_pinn.Engine(cfg)
    eng.set_params(bench.reference_init(layers, seed=0))
    xd = torch.as_tensor(X, device="cuda")
    eng.bind_points(xd)
    return eng, xd


def timed(eng, n):
    """(host enqueue, total) per step, in microseconds"""
    eng.synchronize(); t0 = time.perf_counter(); eng.run(n); t1 = time.perf_counter(); eng.synchronize()
    return (t1 - t0) * 1e6 / n, (time.perf_counter() - t0) * 1e6 / n


def interleaved(eng, n, reps):
    """reps runs without and with the keeper, alternating; the keeper is re-armed each time (a bind costs nothing inside the timed run)"""
    off, on = [], []
    for _ in range(reps):
        eng.clear_keeper()
        off.append(timed(eng, n))
        eng.bind_keeper("res_rms")
        on.append(timed(eng, n))
    st = eng.keeper_state()
    eng.clear_keeper()
    med = lambda v, k: float(np.median([t[k] for t in v]))
    return (med(off, 0), med(off, 1)), (med(on, 0), med(on, 1)), st


say(f"device {torch.cuda.get_device_name(0)}   median of {a.reps} runs each, interleaved")
layers = [2, 64, 64, 64, 64, 1]
X, dv = grid2d(a.points)
eng, xd = engine(layers, X, dv)
eng.bind_monitor(xd, every=100, dv=dv)
eng.run(100); eng.synchronize()
off, on, st = interleaved(eng, a.steps, a.reps)
say(f"{X.shape[0]} points, monitor of {X.shape[0]} points every 100, {a.steps} steps: {off[1] / 1e3:.4f} ms/step without keeper, {on[1] / 1e3:.4f} ms/step with "
    f"(difference {on[1] - off[1]:+.2f} us/step; P = {eng.n_params} floats copied on an improvement; last run: {st})")
eng.close()

X, dv = grid2d(3969)
eng, xd = engine(layers, X, dv)
Xm, dvm = grid2d(16384)
xm = torch.as_tensor(Xm, device="cuda")
eng.bind_monitor(xm, every=100, dv=dvm)
eng.run(200); eng.synchronize()
off, on, st = interleaved(eng, a.small_steps, a.reps)
say(f"{X.shape[0]} points (graph replay), {Xm.shape[0]}-point monitor every 100, {a.small_steps} steps: host enqueue {off[0]:.2f} us/step, total {off[1]:.2f} us/step "
    f"without keeper; {on[0]:.2f} / {on[1]:.2f} us/step with (difference {on[1] - off[1]:+.2f} us/step; last run: {st})")
eng.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
