"""What engine creation decides, cell by cell: for every class of the switch matrix (tests/test_gpu_switch_matrix.py::CLASSES, each of
its batches) the default environment and every value of tests/switch_table.py that applies to the class -- the path, the parameter
count and the active_kernels strings of the engine created under it.  tools/create_table.py writes them to
tests/golden/create_table.json from a build of the commit before a change to creation; tests/test_gpu_create_table.py holds the build
under test to that file.  No step runs: 64 collocation points (3 for the large-batch stand-ins) and 5 boundary points are bound, which
is all active_kernels needs -- creation never sees the batch size, and the size-dependent strings are tests/test_gpu_seams.py's."""
import numpy as np

from oracle import gpe_oracle as go
from tests import switch_table as T
from tests import test_gpu_switch_matrix as M

N_POINTS, N_STAND_IN, N_BOUNDARY = 64, 3, 5


def key(name, bi, env):
    return f"{name}[{bi}] " + (" ".join(f"{k}={v}" for k, v in sorted(env.items())) or "default")


def cells():
    """{key: (class, batch index, environment)}: no cell left out, none twice (two rows may name the same combination)"""
    out = {}
    for name, bi in M.CELLS:
        d = M.descriptor(name, bi)
        base = M.CLASSES[name][1][bi][1]
        envs = [dict(base)] + [dict(base, **val) for row in T.SWITCHES.values() if row["applies_to"](d) for val in row["values"]]
        for env in envs:
            out[key(name, bi, env)] = (name, bi, env)
    return out


def record(name, bi, env):
    """create the engine of the cell under `env`, bind the points, read what creation decided"""
    import torch
    kw, batches, _, _, n_orth = M.CLASSES[name]
    n = N_STAND_IN if batches[bi][2] is not None else N_POINTS
    d = kw["layers"][0]
    rng = np.random.default_rng(1)
    x = (np.linspace(-6, 6, n).reshape(-1, 1) if d == 1 else rng.uniform(-3, 3, (n, d))).astype(np.float32)
    x_bc = (np.linspace(-6, 6, N_BOUNDARY).reshape(-1, 1) if d == 1 else rng.uniform(-3, 3, (N_BOUNDARY, d))).astype(np.float32)
    flat = np.zeros(go.param_count(kw["layers"], kw.get("net_kind", 0)), np.float32)
    orth = np.ones((n_orth, n)) if n_orth else None
    with M.environment(env):
        try:
            eng = M.make(name, n, x, flat, x_bc, orth)
        except (ValueError, RuntimeError) as ex:          # (a refusal is a decision of creation too)
            return {"refused": str(ex)}
        try:
            return {"path": eng.active_path, "params": eng.n_params, "kernels": eng.active_kernels}
        finally:
            eng.close()
            torch.cuda.synchronize()
