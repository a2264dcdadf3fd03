"""Per-point quadrature weights and graded stratified sets, the parts that need no GPU: the weighted fp64 reference against the oracle
(tests/weighted_ref.py) and the numpy restatement of the graded sampler (gpe_pinn/sampler.py)."""
import dataclasses

import numpy as np
import pytest

from gpe_pinn import sampler as S
from oracle import gpe_oracle as go
from tests import helpers as H
from tests.weighted_ref import duplicated, weighted_loss_and_grad

N = 37
FLAVOURS = {
    "plain": dict(layers=[2, 16, 16, 1], gamma=10.0, dx=0.05),
    "riesz_variational": dict(layers=[2, 16, 16, 1], gamma=50.0, w_riesz=2.0, riesz_kind=go.RIESZ_VARIATIONAL, dx=0.05),
    "energy_lambda_regs": dict(layers=[2, 16, 16, 1], gamma=20.0, kinetic_coeff=1.0, pot_scale=1.0, w_norm=0.0, lambda_kind=go.LAMBDA_ENERGY,
                               w_reg_f=1.0, w_reg_lam=1.0, dx=1.0),
    "orth": dict(layers=[2, 16, 16, 1], gamma=10.0, w_orth=3.0, dx=0.05),
    "complex_rot": dict(layers=[2, 16, 16, 2], complex_psi=True, gamma=30.0, omega_rot=0.8, dx=0.02),
    "1d_base_merged_bc": dict(layers=[1, 16, 16, 1], gamma=2.0, base_mode=1, dx=0.03),
}


def _case(name):
    kw = FLAVOURS[name]
    rng = np.random.default_rng(5)
    d = kw["layers"][0]
    x = np.linspace(-6, 6, N).reshape(-1, 1) if d == 1 else rng.uniform(-3, 3, (N, d))
    flat = rng.normal(0, 1, go.param_count(kw["layers"])) * 0.4
    x_bc = np.array([[-6.0], [6.0]]) if name == "1d_base_merged_bc" else None
    orth = rng.normal(0, 1, (1, N)) if name == "orth" else None
    pb = go.Problem(**kw) if x_bc is not None else go.Problem(**kw, w_bc=0.0)
    return pb, flat, x, x_bc, orth


def _agree(a, b, tol=1e-12):
    (sa, ga, _), (sb, gb) = a, b
    for k in ("loss", "mu"):
        assert abs(sa[k] - sb[k]) <= tol * max(abs(sb[k]), 1e-300), (k, sa[k], sb[k])
    assert H.rel_err(ga, gb) <= tol


@pytest.mark.parametrize("name", sorted(FLAVOURS))
def test_weighted_ref_with_unit_weights_is_the_oracle(name):
    pb, flat, x, x_bc, orth = _case(name)
    sc, grad, _ = go.full_loss_and_grad(pb, flat, x, x_bc, orth=orth)
    _agree(weighted_loss_and_grad(pb, flat, x, np.ones(N), x_bc, orth=orth), (sc, grad))


@pytest.mark.parametrize("name", sorted(FLAVOURS))
def test_weighted_ref_with_integer_weights_is_the_oracle_on_the_duplicated_batch(name):
    pb, flat, x, x_bc, orth = _case(name)
    q = np.random.default_rng(8).integers(1, 4, N).astype(np.float64)
    xd, od = duplicated(x, q, orth)
    sc, grad, _ = go.full_loss_and_grad(dataclasses.replace(pb, n_global=int(q.sum())), flat, xd, x_bc, orth=od)
    ref = weighted_loss_and_grad(pb, flat, x, q, x_bc, orth=orth)
    _agree(ref, (sc, grad))
    assert ref[0]["sum_r2"] == pytest.approx(sc["pde"] * q.sum(), rel=1e-12)


def test_weighted_ref_drops_a_zero_weight_point_at_the_same_W():
    pb, flat, x, _, _ = _case("plain")
    q = np.random.default_rng(2).uniform(0.25, 4, N)
    q[::7] = 0.0
    keep = q > 0
    a = weighted_loss_and_grad(pb, flat, x, q)
    b = weighted_loss_and_grad(pb, flat, x[keep], q[keep], W=q.sum())
    _agree(a, (b[0], b[1]))


# ---- graded stratified sets ---------------------------------------------------------------------------------------------------------
EDGES = {1: [S.sinh_edges(6.0, 257, 2.0)], 2: [S.sinh_edges(4.0, 17, 2.5), S.sinh_edges(3.0, 19, 1.0)],
         3: [S.sinh_edges(4.0, 5, 1.5), S.sinh_edges(3.0, 7, 2.0), S.sinh_edges(2.0, 9, 0.5)]}


@pytest.mark.parametrize("d", [1, 2, 3])
def test_graded_points_lie_in_their_cells_and_blocks_are_rows_of_the_full_set(d):
    ed = EDGES[d]
    shape = tuple(a.size - 1 for a in ed)
    full = S.graded_points(ed, seed=11, draw=3)
    assert full.dtype == np.float32 and full.shape == (int(np.prod(shape)), d)
    idx = np.unravel_index(np.arange(full.shape[0]), shape)
    for k in range(d):                                      # closed cell of first_cell + j on every axis (default clip: the end edges)
        assert np.all(full[:, k] >= ed[k][idx[k]]) and np.all(full[:, k] <= ed[k][idx[k] + 1])
    for first, n in ((0, 1), (1, 17), (full.shape[0] - 18, 18), (5, full.shape[0] - 5)):
        blk = S.graded_points(ed, seed=11, draw=3, first_cell=first, n=n)
        assert np.array_equal(blk.view(np.uint32), full[first:first + n].view(np.uint32))
    other = S.graded_points(ed, seed=11, draw=4)
    assert not np.array_equal(other, full)
    assert not np.array_equal(S.graded_points(ed, seed=12, draw=3), full)


def test_graded_clip_clamps():
    ed = EDGES[2]
    clip = ([-1.0, -0.5], [1.5, 0.25])
    x = S.graded_points(ed, seed=1, draw=0, clip=clip)
    raw = S.graded_points(ed, seed=1, draw=0)
    lo, hi = np.float32(clip[0]), np.float32(clip[1])
    assert np.array_equal(x, np.minimum(np.maximum(raw, lo), hi))
    assert (x == lo).any() and (x == hi).any() and np.all(x >= lo) and np.all(x <= hi)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_graded_weights_are_the_axis_order_fp32_product_of_widths(d):
    ed = EDGES[d]
    shape = tuple(a.size - 1 for a in ed)
    q = S.graded_weights(ed)
    idx = np.unravel_index(np.arange(q.size), shape)
    want = None
    for k in range(d):
        w = np.float32(ed[k][idx[k] + 1]) - np.float32(ed[k][idx[k]])
        want = w if want is None else np.float32(want * w)
    assert q.dtype == np.float32 and np.array_equal(q, want) and np.all(q > 0)
    W = S.graded_total(ed)
    assert abs(W - q.sum(dtype=np.float64)) <= 1e-6 * W
    assert np.array_equal(S.graded_weights(ed, first_cell=3, n=2), q[3:5])
    # neither depends on the draw: they are functions of the edges alone (no seed / draw argument), and the points of two draws share them
    for draw in (0, 9):
        x = S.graded_points(ed, seed=4, draw=draw)
        for k in range(d):
            assert np.all(x[:, k] >= ed[k][idx[k]]) and np.all(x[:, k] <= ed[k][idx[k] + 1])


def test_sinh_edges():
    for cells in (1, 2, 5, 16, 257):
        for stretch in (0.0, 0.5, 3.0):
            e = S.sinh_edges(4.0, cells, stretch)
            assert e.dtype == np.float32 and e.size == cells + 1
            assert np.all(e[1:] > e[:-1])
            assert np.array_equal(e, -e[::-1])
            assert e[0] == np.float32(-4.0) and e[-1] == np.float32(4.0)
    uni = np.linspace(-4, 4, 17)
    assert np.abs(S.sinh_edges(4.0, 16, 0.0) - uni).max() <= 4 * 2.0 ** -24 * 4
    assert np.abs(S.sinh_edges(4.0, 16, 1e-4) - uni).max() <= 1e-7 + 4 * 1e-8       # sinh(s t)/sinh(s) = t (1 + O(s^2))
    w = np.diff(S.sinh_edges(4.0, 16, 3.0))
    assert w[7] < w[0] / 5                                                             # refined towards the centre
