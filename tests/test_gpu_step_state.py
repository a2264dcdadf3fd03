"""Entry points mixed on one live engine: step(), the three phases, run() (graph replay), residual(), forward() and calls out of order
leave the same parameters and Adam state as the same number of plain step() calls -- what one step leaves in the engine's per-step
record must not reach the next sequence.  The boundary batch runs in launches of its own (GPE_MERGE_BC=0), through the side stream."""
import os

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import capi
from oracle import gpe_oracle as go
from tests.test_gpu_parity import _inputs, make_engine

pytestmark = pytest.mark.gpu

LAYERS = [1, 32, 32, 32, 1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _state(eng):
    m, v, step = eng.get_adam_state()
    return eng.get_params(), m, v, step


def _same_state(a, b):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]


def _engines(N, count=2):
    """`count` equal engines on N collocation and two boundary points, created under GPE_MERGE_BC=0"""
    kw = dict(layers=LAYERS, activation=1, kinetic_coeff=1.0, pot_scale=1.0, gamma=5.0, base_mode=0, perturb_scale=0.05, dx=12 / (N - 1))
    x, flat, x_bc = _inputs(kw, N)
    old = os.environ.get("GPE_MERGE_BC")
    os.environ["GPE_MERGE_BC"] = "0"
    try:
        return [make_engine(go.Problem(**kw), flat, x, x_bc) for _ in range(count)]
    finally:
        if old is None:
            os.environ.pop("GPE_MERGE_BC", None)
        else:
            os.environ["GPE_MERGE_BC"] = old


def _raises_state_and_changes_nothing(eng, fn):
    before = _state(eng)
    with pytest.raises(gpe_pinn.GPEError) as ei:
        fn()
    assert ei.value.code == capi.GPE_ERR_STATE, (ei.value.code, str(ei.value))
    assert _same_state(_state(eng), before)


def _phases(eng):
    eng.step_begin(); eng.step_backward(); eng.step_update()


def test_mixed_entry_points_with_the_head_in_its_own_kernel():
    """7 000 points: between 6 145 and 32 768 the head sums are formed by k_head_pde in step() and in the phases alike, so both engines
    run the same kernels in the same order: parameters, Adam moments and step counter bit for bit; the history loss to 1e-10
    relative (the reported loss carries one atomically summed fp64 term)."""
    X, Y = _engines(7000)
    assert ",head" not in X.active_kernels["fwd"], X.active_kernels
    X.step()
    _phases(X)
    _raises_state_and_changes_nothing(X, X.step_update)
    X.residual()
    X.run(8)
    _phases(X)
    X.step()
    Y.step(); Y.step()
    Y.residual()
    for _ in range(10):
        Y.step()
    sx, sy = _state(X), _state(Y)
    assert sx[3] == sy[3] == 12
    assert _same_state(sx, sy), [int((_bits(p) != _bits(q)).sum()) for p, q in zip(sx[:3], sy[:3])]
    lx = np.array([h["loss"] for h in X.read_history(1, 12)])
    ly = np.array([h["loss"] for h in Y.read_history(1, 12)])
    assert np.all(np.abs(lx - ly) <= 1e-10 * np.abs(ly)), (lx, ly)
    X.close(); Y.close()


def test_mixed_entry_points_with_head_and_seeds_fused_into_whole_steps():
    """2 048 points: whole steps run the head in the cooperative forward kernel and form the seeds in f_backward_pipe.  Neither a
    refused call, residual(), a graph replay nor a forward pass on other points between them changes what they compute."""
    X, Y = _engines(2048)
    assert X.active_kernels["fwd"].endswith(",head>") and "f_backward_pipe" in X.active_kernels["bwd"] and \
        X.active_kernels["bwd"].endswith(",seeds>"), X.active_kernels
    X.step()
    _raises_state_and_changes_nothing(X, X.step_backward)
    X.residual()
    X.run(8)
    other = torch.linspace(-5.0, 5.0, 100, device="cuda").reshape(-1, 1)
    assert torch.isfinite(X.forward(other)).all()
    X.step()
    Y.step()
    Y.residual()
    for _ in range(9):
        Y.step()
    sx, sy = _state(X), _state(Y)
    assert sx[3] == sy[3] == 10
    assert _same_state(sx, sy), [int((_bits(p) != _bits(q)).sum()) for p, q in zip(sx[:3], sy[:3])]
    X.close(); Y.close()
