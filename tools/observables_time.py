#!/usr/bin/env python3
"""Cost of the device-side observables and of the held-out monitor.

(1) Engine.observables on the bound grid against the host-side way of getting the same numbers (forward_jets + copy + numpy sums, what
    tools/accuracy_cfg4.py:state_numbers did): HIP-event / wall time, median of repeated calls.
(2) gpe_run step time with a monitor of the training grid's size at every = 100 against gpe_run without one, same process, same box.
(3) the small-batch case (4 000 points, graph replay): host time per step with and without the monitor (cut replays).

usage: python tools/observables_time.py [--points 1048576 --steps 300 --reps 9 --out profiles/r05/observables_time.txt]
For the per-kernel numbers run this under `rocprofv3 --kernel-trace --stats -- python tools/observables_time.py --only obs`."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import gpe_pinn
from gpe_pinn import capi

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=1 << 20)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--only", default="", help="obs: part (1) only")
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


def engine(layers, X, dv, **kw):
    import bench
    cfg = gpe_pinn.GPEConfig(layers=layers, gamma=kw.pop("gamma", 500.0), dx=dv, w_bc=0.0, lr=1e-4, sched=capi.SCHED_CONST, history_capacity=8, **kw)
    eng = gpe_pinn.Engine(cfg)
    eng.set_params(bench.reference_init(layers, seed=0))
    xd = torch.as_tensor(X, device="cuda")
    eng.bind_points(xd)
    return eng, xd


def host_way(eng, xd, X, dv, cplx, g):
    J = eng.forward_jets(xd).cpu().numpy().astype(np.float64)
    rho = (J[0] ** 2).sum(axis=1)
    I = dv * rho.sum()
    kin = 0.5 * dv * (J[1] ** 2 + J[2] ** 2).sum()
    pot = dv * (0.5 * (X.astype(np.float64) ** 2).sum(axis=1) * rho).sum()
    inter = 0.5 * g * dv * (rho * rho).sum()
    return (kin + pot) / I + inter / I ** 2, I


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append((e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))
    ev, wall = np.median([t[0] for t in ts]), np.median([t[1] for t in ts])
    return float(ev), float(wall)


say(f"device {torch.cuda.get_device_name(0)}")
for name, layers, npts, kw in (("ns_2d_4x64", [2, 64, 64, 64, 64, 1], a.points, {}),
                               ("cfg4_2d_6x128_rot", [2, 128, 128, 128, 128, 128, 128, 2], 65536, dict(complex_psi=True, omega_rot=0.8))):
    X, dv = grid2d(npts)
    eng, xd = engine(layers, X, dv, **kw)
    eng.observables(); host_way(eng, xd, X, dv, bool(kw), 500.0)        # warm-up: allocations
    ev, wall = median_ms(lambda: eng.observables(), a.reps)
    hev, hwall = median_ms(lambda: host_way(eng, xd, X, dv, bool(kw), 500.0), max(3, a.reps // 3))
    o = eng.observables()
    E_host, I_host = host_way(eng, xd, X, dv, bool(kw), 500.0)
    say(f"{name} {X.shape[0]} points: Engine.observables {ev:.3f} ms (HIP events; host wall {wall:.3f} ms)   forward_jets + copy + numpy {hwall:.1f} ms wall "
        f"  [E - Omega Lz part excluded: E_kin+pot+int device {o['kin'] + o['pot'] + o['inter']:.9f} host {E_host:.9f}, norm {o['norm']:.9f} / {I_host:.9f}]")
    if a.only != "obs" and name == "ns_2d_4x64":
        def run_ms(n):
            torch.cuda.synchronize(); t0 = time.perf_counter(); eng.run(n); t1 = time.perf_counter(); eng.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n, (t1 - t0) * 1e3 / n
        eng.run(20); eng.synchronize()
        base = [run_ms(a.steps)[0] for _ in range(3)]
        eng.bind_monitor(xd, every=100, dv=dv)
        mon = [run_ms(a.steps)[0] for _ in range(3)]
        eng.clear_monitor()
        base2 = [run_ms(a.steps)[0] for _ in range(3)]
        say(f"   gpe_run step time: no monitor {np.median(base):.4f} ms, monitor of {X.shape[0]} points every 100 {np.median(mon):.4f} ms, no monitor again {np.median(base2):.4f} ms "
            f"(expected + observables/100 = {ev / 100:.4f} ms)")
    eng.close()
if a.only != "obs":
    X, dv = grid2d(4000)
    eng, xd = engine([2, 64, 64, 64, 64, 1], X, dv)
    Xm, dvm = grid2d(16384)
    xm = torch.as_tensor(Xm, device="cuda")

    def host_us(n):
        eng.synchronize(); t0 = time.perf_counter(); eng.run(n); t1 = time.perf_counter(); eng.synchronize()
        return (t1 - t0) * 1e6 / n, (time.perf_counter() - t0) * 1e6 / n
    eng.run(64); eng.synchronize()
    b = [host_us(2000) for _ in range(3)]
    eng.bind_monitor(xm, every=100, dv=dvm)
    m = [host_us(2000) for _ in range(3)]
    eng.clear_monitor()
    say(f"small batch {X.shape[0]} points (graph replay), 2000 steps: host enqueue {np.median([v[0] for v in b]):.2f} us/step, total {np.median([v[1] for v in b]):.2f} us/step without monitor; "
        f"{np.median([v[0] for v in m]):.2f} / {np.median([v[1] for v in m]):.2f} us/step with a {Xm.shape[0]}-point monitor every 100 (replays cut at the monitor steps)")
    eng.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
