"""Time per L-BFGS tick with the strong-Wolfe line search beside the time per iteration without it, on the north-star network
([2,64,64,64,64,1], gamma 500, physics loss) at 4 096 and 65 536 collocation points, history 10 and 100.  Wall clock around gpe_lbfgs_run(50) and a
synchronisation (the launches are enqueued back to back), medians [min .. max] of 7 interleaved blocks after the rings have filled.  Writes the table to stdout; profiles/lbfgs_ls/step_time.txt keeps it.

    python tools/lbfgs_tick_time.py"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpe_pinn import GPEConfig, Engine  # noqa: E402
from bench import reference_init  # noqa: E402

LAYERS, HALF, BLOCK, BLOCKS = [2, 64, 64, 64, 64, 1], 8.0, 50, 7


def engine(n, history, ls):
    side = int(round(n ** 0.5))
    g = np.linspace(-HALF, HALF, side, dtype=np.float64)
    x = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    eng = Engine(GPEConfig(layers=LAYERS, gamma=500.0, dx=(2 * HALF / side) ** 2, w_bc=0.0))
    eng.set_params(reference_init(LAYERS, seed=1))
    eng.bind_points(torch.as_tensor(x, device="cuda"))
    # a small step keeps both runs in the smooth part of the loss for the whole measurement: no freeze, no skip
    eng.lbfgs_config(1e-3, history=history, tolerance_grad=0.0, tolerance_change=0.0, line_search="strong_wolfe" if ls else None)
    eng.lbfgs_run(history + 20)
    eng.synchronize()
    return eng


def block(eng):
    eng.synchronize()
    t0 = time.perf_counter()
    eng.lbfgs_run(BLOCK)
    eng.synchronize()
    return (time.perf_counter() - t0) / BLOCK * 1e6


def main():
    for n in (4096, 65536):
        for history in (10, 100):
            engs = {ls: engine(n, history, ls) for ls in (False, True)}
            times = {ls: [] for ls in engs}
            for _ in range(BLOCKS):
                for ls, e in engs.items():
                    times[ls].append(block(e))
            rec, lsr = engs[True].lbfgs_read(), engs[True].lbfgs_ls_read()
            plain, tick = np.median(times[False]), np.median(times[True])
            print(f"points {n:6d}  history {history:3d}  iteration without line search {plain:8.1f} us [{min(times[False]):.1f} .. {max(times[False]):.1f}]   "
                  f"tick with strong Wolfe {tick:8.1f} us [{min(times[True]):.1f} .. {max(times[True]):.1f}]   "
                  f"({tick - plain:+.1f} us, {100 * (tick / plain - 1):+.1f} %)   accepted {lsr['accepted']} of {lsr['evals_total']} evaluations, "
                  f"pairs held {rec['count']}, frozen {rec['frozen']} / {engs[False].lbfgs_read()['frozen']}")
            for e in engs.values():
                e.close()


if __name__ == "__main__":
    main()
