#!/usr/bin/env python
"""profiles/seams/seams_time.txt from a run of tests/test_gpu_seams.py:

    SEAMS_REPORT=seams.json python -m pytest tests/test_gpu_seams.py -m gpu -q --durations=5 | tee seams.log
    python tools/seam_figures.py seams.json seams.log > profiles/seams/seams_time.txt

Per cell (class, bound points): the engine's relative errors against the fp64 oracle as the module recorded them, and beside
them the oracle's own float32 run against its float64 self on the same inputs (computed here, on the host)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import helpers as H          # noqa: E402
from tests import seam_ref as R         # noqa: E402


def main(report, log=None):
    rec = json.load(open(report))
    print("tests/test_gpu_seams.py on one MI355X; fp64 oracle references on the host included in every time.")
    if log:
        tail = [l.rstrip() for l in open(log) if " passed" in l or " failed" in l or "s call " in l]
        print("\n".join(tail))
    print(f"{len(rec)} cells (class, bound points; a test runs both sides of a seam, cells on one size are shared); slowest cell: "
          + max(rec, key=lambda k: rec[k]["seconds"]) + f" {max(r['seconds'] for r in rec.values()):.2f} s")
    print("\nRelative errors against the fp64 oracle: engine | the oracle's own float32 run.  Records, not bounds (bounds: mu 2e-5, loss 1e-4,")
    print("gradient 5e-5 of the maximum, whole and per parameter block).\n")
    print(f"{'class-bound points':22s} {'mu':>17s} {'loss':>17s} {'gradient':>17s} {'worst block':>17s}  kernels")
    f32 = {}
    for key, r in rec.items():
        cls, n = key.split("-")[0], int(key.split("-")[1])
        if (cls, n) not in f32:
            pb = R.problem(cls)
            s64, g64 = R.step(cls, n, np.float64)
            s32, g32 = R.step(cls, n, np.float32)
            f32[(cls, n)] = dict(mu=abs(s32["mu"] - s64["mu"]) / abs(s64["mu"]), loss=abs(s32["loss"] - s64["loss"]) / abs(s64["loss"]),
                                 grad=H.rel_err(g32, g64), block=max(H.block_rel_errs(g32, g64, H.param_blocks(pb.layers, pb.net_kind)).values()))
        o = f32[(cls, n)]
        print(f"{key:22s} " + " ".join(f"{r[k]:8.1e}|{o[k]:8.1e}" for k in ("mu", "loss", "grad", "block")) + f"  {r['kernels']}", flush=True)


if __name__ == "__main__":
    main(*sys.argv[1:3])
