#!/usr/bin/env python
"""Host time of gpe_create + gpe_destroy for the NS 2D [2,64x4,1] configuration: PAIRS pairs (default 20) after one untimed pair that
loads the code objects.  GPE_HIP_LIB selects another build of the library (the parent commit's, for a before / after).

    python tools/create_time.py [PAIRS]
"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpe_pinn              # noqa: E402
from gpe_pinn import capi    # noqa: E402


def main(pairs=20):
    lib = capi.load()
    cfg = gpe_pinn.GPEConfig(layers=[2, 64, 64, 64, 64, 1], gamma=500.0).to_c()

    def pair():
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.gpe_create(C.byref(cfg), 0, None, C.byref(h))
        assert rc == capi.GPE_OK, (rc, lib.gpe_last_error(None))
        lib.gpe_destroy(h)
        return (time.perf_counter() - t0) * 1e3

    first = pair()
    ts = sorted(pair() for _ in range(pairs))
    print(f"gpe_create + gpe_destroy, {pairs} pairs: mean {sum(ts) / pairs:.4f} ms, median {ts[pairs // 2]:.4f}, min {ts[0]:.4f}, max {ts[-1]:.4f} "
          f"(first, untimed: {first:.1f} ms)", flush=True)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
