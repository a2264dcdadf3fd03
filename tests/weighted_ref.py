"""fp64 reference for a collocation batch with per-point quadrature weights (include/gpe_hip.h: gpe_bind_weights), built from the
oracle's own arithmetic: its two-phase data-parallel protocol with ONE point per shard.

Phase 1 gives every point's local sums; the totals are sum_i q_i * sums_i.  Phase 2 with those totals gives every point's gradient and
r^2; the batch's are sum_i q_i * (...).  N of the means is W = sum q (Problem.n_global takes a float).  With integer weights this is
the oracle on the batch with row i repeated q_i times (tests/test_weights_cpu.py holds it to that, to 1e-12), so any q -- real-valued
or zero -- has a reference that is the oracle's arithmetic and nothing else.  The boundary term has no weight: it is formed once."""
import dataclasses

import numpy as np

from oracle import gpe_oracle as go


def weighted_loss_and_grad(pb, flat, x, q, x_bc=None, bc_target=None, orth=None, W=None):
    """-> (scalars as go.assemble gives them plus num / den / sum_r2 / integral, gradient, dict(psi, residual) per point).
    x [N, d], q [N] >= 0, orth [n_orth, N] or None; W: sum of q over all ranks (None: over this batch)."""
    x = np.asarray(x, np.float64)
    q = np.asarray(q, np.float64).ravel()
    flat = np.asarray(flat, np.float64)
    N = x.shape[0]
    assert q.shape == (N,) and np.all(q >= 0)
    W = float(q.sum()) if W is None else float(W)
    pbw = dataclasses.replace(pb, n_global=W)
    sl = (lambda i: None) if orth is None else (lambda i: np.asarray(orth, np.float64)[:, i:i + 1])
    parts = [go.loss_and_grad(pbw, flat, x[i:i + 1], orth=sl(i), phase=1) for i in range(N)]
    tot = {k: float(sum(q[i] * parts[i][k] for i in range(N))) for k in parts[0]}
    grad, sr2, res0 = None, 0.0, None
    psi = np.zeros((N, pb.n_out)); resid = np.zeros((N, pb.n_out))
    for i in range(N):
        r = go.loss_and_grad(pbw, flat, x[i:i + 1], x_bc if i == 0 else None, bc_target if i == 0 else None, orth=sl(i), shard_sums=tot)
        if i == 0:
            res0, grad = r, r["grad_bc"].copy()
        grad += q[i] * r["grad_local"]
        sr2 += q[i] * r["sum_r2"]
        psi[i], resid[i] = r["psi"][0], r["residual"][0]
    sc = go.assemble(pbw, res0, sum_r2_total=sr2, n_global=W)
    sc.update(num=tot["num"], den=tot["den"], sum_r2=sr2, integral=res0["integral"])
    return sc, grad, dict(psi=psi, residual=resid)


def duplicated(x, q, *rows):
    """The batch with row i repeated q_i times (integer q): (x_dup, *rows_dup); rows are arrays whose LAST axis runs over the points."""
    rep = np.asarray(q).astype(np.int64)
    assert np.array_equal(rep, np.asarray(q))
    idx = np.repeat(np.arange(len(rep)), rep)
    return (np.asarray(x)[idx],) + tuple(None if r is None else np.asarray(r)[..., idx] for r in rows)
