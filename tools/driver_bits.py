#!/usr/bin/env python3
"""Step-driver BITS: every entry point that drives a step from the reverse pass to the next forward pass (step, run with and without the
captured graph, the split phases, residual between steps, the pre-training steps, L-BFGS with and without the line search and the
monitor, the data-parallel step at world 1 in its inline, two-stream, bucketed and stale-gradient forms, the update-kernel switches, the
mixture's forward-only detour, the optimiser-state setters), one line per cell: active_kernels, each loss as a hex float (of a run its
first step's, out of the history, and its last; an L-BFGS run is split 1 + (n - 1) for the same reason), a sha256 over parameters,
gradient, Adam moments, step count and the history window (and whatever else the cell read), and the monitor's records where
one is bound.  Networks: [2,64,64,64,64,1] (P = 12 737: the register-cached single-workgroup update), [2,128,128,128,1] (P = 33 537: the
multi-workgroup update), [1,32,32,1] with a symmetry term, [2,64,64,1] forced onto the generic set, and a mixture [2,64,64,2]; each on
N = 200 collocation points with 5 boundary points (merged) and with 40 (forked to the side stream).  Run it once per library build
(GPE_HIP_LIB=...) and diff the outputs: a refactor of the drivers reproduces every line that two runs of one build reproduce.
usage: tools/driver_bits.py > bits.txt            tools/driver_bits.py --time     (world-1 run_dp, 4 000 points: us per step)"""
import hashlib, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpe_pinn
from gpe_pinn import capi
from bench import reference_init

COMMON = dict(gamma=10.0, p=3, kinetic_coeff=0.5, pot_scale=0.5, w_bc=10.0, w_norm=20.0, lr=1e-3)
NETS = {
    "h64x4": dict(layers=[2, 64, 64, 64, 64, 1]),
    "h128x3": dict(layers=[2, 128, 128, 128, 1]),
    "sym32": dict(layers=[1, 32, 32, 1], w_sym=1.0),
    "generic": dict(layers=[2, 64, 64, 1], path=capi.PATH_GENERIC),
    "mixture": dict(layers=[2, 64, 64, 2], mixture=True, mix_g=(4.0, 4.0, 2.0), mix_norm=(0.5, 0.5)),
}
N = 200


def dev(a):
    return torch.as_tensor(a, device="cuda")


class Cell:
    """One engine with everything bound, and what the cell's line is made of."""

    def __init__(self, kw, nb, n=N):
        self.kw, self.d = kw, kw["layers"][0]
        rng = np.random.default_rng(1000 * nb + n)
        self.x = ((rng.random((n, self.d)) * 2 - 1) * 4).astype(np.float32)
        xb = ((rng.random((nb, self.d)) * 2 - 1) * 4).astype(np.float32)
        xb[:, 0] = np.float32(4.0)
        self.xm = ((rng.random((64, self.d)) * 2 - 1) * 4).astype(np.float32)          # held-out monitor points
        self.eng = e = gpe_pinn.Engine(gpe_pinn.GPEConfig(dx=8.0 ** self.d / n, **COMMON, **kw))
        e.set_params(reference_init(kw["layers"], seed=1))
        e.bind_points(dev(self.x)); e.bind_boundary(dev(xb))
        self.losses, self.h, self.mon = [], hashlib.sha256(), False

    def loss(self, v):
        self.losses.append(float(v).hex())

    def first_step_loss(self):
        """the first step's loss out of the history: the one loss of a run that no atomic add of an earlier step has touched"""
        self.loss(self.eng.read_history(1, 1)[0]["loss"])

    def put(self, *arrays):
        for a in arrays:
            self.h.update(np.ascontiguousarray(a).tobytes())

    def monitor(self, every):
        (self.eng.bind_mixture_monitor if self.kw.get("mixture") else self.eng.bind_monitor)(dev(self.xm), every)
        self.mon = True

    def target(self):
        r2 = (self.x.astype(np.float64) ** 2).sum(1, keepdims=True)
        self.eng.bind_target(dev(np.repeat(np.exp(-0.5 * r2), self.kw["layers"][-1], 1).astype(np.float32)))

    def line(self):
        e = self.eng
        m, v, step = e.get_adam_state()
        self.put(e.get_params(), e.get_grad(), m, v, np.int64(step))
        if step > 0:
            self.put(e.read_history_array(1, step))
        out = f"{';'.join(f'{a}={b}' for a, b in e.active_kernels.items())} | {' '.join(self.losses)} | {self.h.hexdigest()[:16]}"
        if self.mon:
            rec = (e.read_mixture_monitor_array if self.kw.get("mixture") else e.read_monitor_array)()
            out += f" | monitor {len(rec)} {hashlib.sha256(rec.tobytes()).hexdigest()[:16]}"
        e.close()
        return out


# ---- the cells: name -> (environment, body) ------------------------------------------------------------------------------------------
def steps(k):
    def body(c):
        for _ in range(k):
            c.loss(c.eng.step()["loss"])
    return body


def run(k, monitor=0, sampler=0):
    def body(c):
        if monitor:
            c.monitor(monitor)
        if sampler:
            c.eng.bind_sampler([-4.0] * c.d, [4.0] * c.d, [N] if c.d == 1 else [20, 10], every=sampler, seed=3)
        c.eng.run(k)
        c.first_step_loss(); c.loss(c.eng.read_scalars()["loss"])
    return body


def phases(c):
    for _ in range(4):
        c.eng.step_begin(); c.eng.step_backward(); c.eng.step_update()
        c.loss(c.eng.read_scalars()["loss"])


def residual(c):
    for _ in range(2):
        c.loss(c.eng.step()["loss"])
        sc, psi, res = c.eng.residual()
        c.loss(sc["loss"]); c.put(psi.cpu().numpy(), res.cpu().numpy())


def mse(c):
    c.target()
    for _ in range(4):
        c.loss(c.eng.mse_step()["loss"])
    loss, g = c.eng.mse_loss_grad()
    c.loss(loss); c.put(g)


def lbfgs(k, wolfe=False, monitor=False):
    def body(c):
        c.eng.lbfgs_config(lr=0.5 if wolfe else 1e-2, history=5, line_search="strong_wolfe" if wolfe else None)
        if monitor:
            c.monitor(3); c.eng.lbfgs_monitor(True)
        c.eng.lbfgs_run(1)
        c.loss(c.eng.lbfgs_read()["loss"])
        c.eng.lbfgs_run(k - 1)
        r = c.eng.lbfgs_read()
        c.loss(r["loss"]); c.put(np.array([r[f] for f in c.eng.LBFGS_FIELDS], np.float64), c.eng.lbfgs_point())
    return body


def dp(k, stale=False, run_dp=False):
    def body(c):
        c.eng.comm_init(0, 1)
        if stale:
            c.eng.comm_set_async(True)
        if run_dp:
            c.eng.run_dp(k)
            c.first_step_loss(); c.loss(c.eng.read_scalars()["loss"])
        else:
            for _ in range(k):
                c.eng.step_dp()
                c.loss(c.eng.read_scalars()["loss"])
        c.put(np.int64(c.eng.comm_info()["collectives"]))
    return body


def switch(c):
    steps(4)(c)
    run(16)(c)


def mixture_detour(c):
    c.loss(c.eng.step()["loss"])
    en, ms = c.eng.mixture_energy(), c.eng.mixture_scalars()
    c.put(np.array(list(en.values()) + list(ms.values()), np.float64))
    c.loss(c.eng.step()["loss"])


def opt_state(c):
    e = c.eng
    steps(2)(c)
    m, v, step = e.get_adam_state()
    e.set_adam_state(m * np.float32(0.5), v, step + 3)
    e.set_lr(5e-4)
    c.put(np.array([float(a) for a in e.stop_state()], np.float64), np.int64(e.get_adam_state()[2]))
    steps(2)(c)


CELLS = {
    "step6": ({}, steps(6)),
    "run19": ({}, run(19)),
    "run19_graph0": ({"GPE_GRAPH": "0"}, run(19)),
    "run40_mon12_smp20": ({}, run(40, monitor=12, sampler=20)),
    "phases4": ({}, phases),
    "residual": ({}, residual),
    "mse": ({}, mse),
    "lbfgs6": ({}, lbfgs(6)),
    "lbfgs12_wolfe": ({}, lbfgs(12, wolfe=True)),
    "lbfgs12_wolfe_mon": ({}, lbfgs(12, wolfe=True, monitor=True)),
    "dp4": ({}, dp(4)),
    "dp4_inline0": ({"GPE_DP_INLINE": "0"}, dp(4)),
    "dp5_async": ({}, dp(5, stale=True)),
    "run_dp4": ({}, dp(4, run_dp=True)),
    "fuse_update": ({"GPE_FUSE_UPDATE": "1"}, switch),
    "split_update": ({"GPE_SPLIT_UPDATE": "1"}, switch),
    "update_cache0": ({"GPE_UPDATE_CACHE": "0"}, switch),
    "update_multi_min1": ({"GPE_UPDATE_MULTI_MIN": "1"}, switch),
    "mixture_detour": ({}, mixture_detour),
    "opt_state": ({}, opt_state),
}


def cell(kw, nb, env, body):
    os.environ.update(env)
    try:
        c = Cell(kw, nb)
        body(c)
        return c.line()
    finally:
        for k in env:
            del os.environ[k]


def time_run_dp(n=4000, steps_per_call=200, reps=5):
    """world-1 run_dp on the headline network at n points: us per step, best and median of reps"""
    c = Cell(NETS["h64x4"], 5, n)
    c.eng.comm_init(0, 1)
    c.eng.run_dp(50); c.eng.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        c.eng.run_dp(steps_per_call); c.eng.synchronize()
        t.append((time.perf_counter() - t0) / steps_per_call * 1e6)
    c.eng.close()
    print(f"run_dp world 1, N={n}: min {min(t):.2f} us/step, median {sorted(t)[len(t) // 2]:.2f} us/step  ({reps} x {steps_per_call} steps)", flush=True)


if __name__ == "__main__":
    if "--time" in sys.argv:
        time_run_dp()
        sys.exit(0)
    for net, kw in NETS.items():
        for nb in (5, 40):
            for name, (env, body) in CELLS.items():
                if name == "mixture_detour" and not kw.get("mixture"):
                    continue
                try:
                    print(f"{net} nb={nb} {name}: {cell(kw, nb, env, body)}", flush=True)
                except Exception as ex:          # noqa: BLE001 -- reported per cell
                    print(f"{net} nb={nb} {name}: EXC {str(ex)[:200]}", flush=True)
                    if getattr(ex, "code", None) == capi.GPE_ERR_HIP:      # a device error: nothing more is started on this GPU
                        sys.exit(3)
