#!/usr/bin/env python3
"""Cost of re-drawing the collocation set: the engine's device sampler (Engine.bind_sampler) against the host cycle of 16 jittered
sets tools/accuracy_nd.py:run_epochs drives with bind_points, and against no resampling at all.

    python tools/sampler_bench.py                      per-step time of --steps steps at --every, three configurations, two workloads
    python tools/sampler_bench.py --redraws 40         only binds the sampler at 4 000 / 65 536 / 1 048 576 points and steps with
                                                       every = 1: run it under `rocprofv3 --kernel-trace --stats` for the time of
                                                       k_sampler_draw (tools/sampler_bench.py --trace-csv FILE prints it per size)
One JSON line per measurement on stdout."""
import argparse, csv, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--every", type=int, default=100)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--sets", type=int, default=16)
ap.add_argument("--repeat", type=int, default=3, help="timed passes per configuration; the median is reported, all are listed")
ap.add_argument("--redraws", type=int, default=0)
ap.add_argument("--trace-csv", default="", help="a rocprofv3 kernel trace: print the k_sampler_draw durations grouped by grid size, and exit")
a = ap.parse_args()

if a.trace_csv:
    rows = list(csv.DictReader(open(a.trace_csv)))
    col = {k.lower(): k for k in rows[0]}
    name, t0, t1 = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    gx, wx = col.get("grid_size_x") or col.get("grid_size"), col.get("workgroup_size_x") or col.get("workgroup_size")
    by = {}
    for r in rows:
        if "k_sampler_draw" in r[name]:
            by.setdefault((int(r[gx]), int(r[wx])), []).append((int(r[t1]) - int(r[t0])) / 1e3)
    for (g, w), v in sorted(by.items()):
        v = np.array(v)
        print(json.dumps(dict(kernel="k_sampler_draw", grid_threads=g, workgroup=w, launches=len(v), us_median=float(np.median(v)),
                              us_min=float(v.min()), us_max=float(v.max()))))
    sys.exit(0)

import torch
import gpe_pinn
from gpe_pinn import capi
from gpe_pinn.sampler import node_centred
import bench

WORK = {
    # the north-star workload of bench.py (1 048 576 points) and the reference's 4 000 points on a 1D refine-sized network
    "ns_2d_4x64": dict(layers=[2, 64, 64, 64, 64, 1], nodes=(1024, 1024), half=8.0, gamma=500.0),
    "ref_1d_4000": dict(layers=[1, 64, 64, 64, 1], nodes=(4000,), half=10.0, gamma=5.0),
}


def engine(w):
    d = len(w["nodes"])
    ax = [np.linspace(-w["half"], w["half"], k) for k in w["nodes"]]
    X = np.stack([m.ravel() for m in np.meshgrid(*ax, indexing="ij")], axis=1).astype(np.float32)
    h = ax[0][1] - ax[0][0]
    cfg = gpe_pinn.GPEConfig(layers=w["layers"], gamma=w["gamma"], dx=float(h ** d), w_bc=0.0, sched=capi.SCHED_CONST, history_capacity=8)
    eng = gpe_pinn.Engine(cfg)
    eng.set_params(bench.reference_init(w["layers"]))
    return eng, X, h


if a.redraws > 0:
    for n in (4000, 65536, 1048576):
        eng = gpe_pinn.Engine(gpe_pinn.GPEConfig(layers=[2, 32, 32, 1], gamma=1.0, dx=0.01, w_bc=0.0))
        eng.set_params(bench.reference_init([2, 32, 32, 1]))
        shape = {4000: (50, 80), 65536: (256, 256), 1048576: (1024, 1024)}[n]
        eng.bind_sampler((-8.0, -8.0), (8.0, 8.0), shape, every=1)
        eng.run(a.redraws)
        eng.synchronize()
        print(json.dumps(dict(redraws=a.redraws, points=n, draw=eng.sampler_points()[1])), flush=True)
        eng.close()
    sys.exit(0)

for wname, w in WORK.items():
    d = len(w["nodes"])
    res = {}
    for mode in ("none", "device", "host_cycle"):
        eng, X, h = engine(w)
        xd = torch.as_tensor(X, device="cuda")
        eng.bind_points(xd)
        sets = []
        if mode == "device":
            lo, hi, clip = node_centred([w["half"]] * d, w["nodes"])
            eng.bind_sampler(lo, hi, w["nodes"], every=a.every, seed=1, clip=clip)
        elif mode == "host_cycle":
            rng = np.random.default_rng(1)
            for _ in range(a.sets):
                J = X.astype(np.float64) + rng.uniform(-0.5 * h, 0.5 * h, X.shape)
                sets.append(torch.as_tensor(np.clip(J, -w["half"], w["half"]).astype(np.float32), device="cuda"))

        set_i = [0]

        def go(n_steps):
            if mode != "host_cycle":
                eng.run(n_steps)
                return
            left = n_steps
            while left > 0:                       # tools/accuracy_nd.py:run_epochs (the set index carries over from call to call)
                k = min(left, a.every)
                set_i[0] = (set_i[0] + 1) % len(sets)
                eng.bind_points(sets[set_i[0]])
                eng.run(k)
                left -= k

        go(a.warmup)
        eng.synchronize()
        times = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            go(a.steps)
            eng.synchronize()
            times.append((time.perf_counter() - t0) / a.steps * 1e3)
        res[mode] = float(np.median(times))
        print(json.dumps(dict(workload=wname, points=int(X.shape[0]), mode=mode, steps=a.steps, every=a.every, ms_per_step_median=res[mode],
                              ms_per_step_passes=times)), flush=True)
        eng.close()
        del sets, xd
        torch.cuda.empty_cache()
    print(json.dumps(dict(workload=wname, overhead_device_us_per_step=(res["device"] - res["none"]) * 1e3,
                          overhead_host_cycle_us_per_step=(res["host_cycle"] - res["none"]) * 1e3,
                          overhead_device_pct=(res["device"] / res["none"] - 1) * 100, overhead_host_cycle_pct=(res["host_cycle"] / res["none"] - 1) * 100)), flush=True)
