#!/usr/bin/env python3
"""Observables record BITS: one sha256 of the raw record bytes per cell of tests/test_gpu_observe_instances.py (2 kinds x 3 dims x weighted
or not x 3 sizes), of a monitor ring behind run() under graph replay and under plain launches (scalar and mixture), and of a kept record.
Fixed seeds, fixed parameters, no training needed.  Run it once per library build (GPE_HIP_LIB=...) and diff the outputs: a change of
the reduction chain that is a refactor reproduces every hash.   usage: tools/observe_record_bits.py > bits.txt"""
import hashlib, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import gpe_oracle as go
from tests import mixture_cases as mc
from tests import observe_cells as oc
from tests.test_gpu_mixture import dev, make_engine as make_mixture
from tests.test_gpu_parity import _inputs, make_engine


def sha(d):
    """a record dict, or a list of them, as the doubles the library wrote"""
    recs = d if isinstance(d, list) else [d]
    return hashlib.sha256(np.array([v for r in recs for k in r for v in np.ravel(r[k])], np.float64).tobytes()).hexdigest()[:16]


for name in oc.SCALAR:
    for N in oc.SIZES:
        print(f"scalar {name} N {N}: plain {sha(oc.scalar_cell(name, N, False)[-1])} weighted {sha(oc.scalar_cell(name, N, True)[-1])}", flush=True)
for d in (1, 2, 3):
    for N in oc.SIZES:
        print(f"mixture {d}d N {N}: plain {sha(oc.mixture_cell(d, N, False)[-1])} weighted {sha(oc.mixture_cell(d, N, True)[-1])}", flush=True)

# a monitor ring of 5 records behind run(30), a keeper on it: graph replay (cut at the monitor steps) and plain launches
held = np.random.default_rng(5).uniform(-2, 2, (301, 2)).astype(np.float32)
for mode in ("1", "0"):
    os.environ["GPE_GRAPH"] = mode
    kw = dict(layers=[2, 64, 64, 64, 1], gamma=50.0, dx=0.01)
    x, flat, _ = _inputs(kw, 777)
    eng = make_engine(go.Problem(**kw), flat, x, None)
    eng.bind_monitor(dev(held), every=6, dv=16.0 / 301)
    eng.bind_keeper("res_rms")
    eng.run(30)
    print(f"scalar run(30) GPE_GRAPH={mode}: ring {sha(eng.read_monitor())} kept {sha(eng.best_record())} {eng.keeper_state()}", flush=True)
    eng.close()
    layers = [2, 64, 64, 64, 2]
    x, flat, x_bc, tgt = mc.inputs(layers, 777, seed=4)
    eng = make_mixture(mc.problem(layers, 777), flat, x, x_bc, tgt, "auto")
    eng.bind_mixture_monitor(dev(held), every=6, dv=16.0 / 301)
    eng.bind_mixture_keeper("energy")
    eng.run(30)
    print(f"mixture run(30) GPE_GRAPH={mode}: ring {sha(eng.read_mixture_monitor())} kept {sha(eng.best_record())} {eng.keeper_state()}", flush=True)
    eng.close()
