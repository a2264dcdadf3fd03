"""CPU companion of tests/test_gpu_dp_matrix.py: before the GPU is asked to be additive over the explicit world-3 and world-8 cuts
(1-point shards included), the fp64 reference itself is -- its per-shard sums and gradients, added in float64 in rank order, give the
whole-batch call to 1e-12 relative."""
import numpy as np
import pytest

from oracle import gpe_oracle as go
from tests import helpers as H
from tests.test_gpu_parity import CASES, _inputs, _scale

WORLDS = (3, 8)
# one real psi, one complex psi, one energy-functional lambda with both regularisers
ADDITIVE = ["2d_64x4_g500", "2d_complex_rot_variational", "2d_class_loss_64x4"]


@pytest.mark.parametrize("world", WORLDS)
def test_explicit_cuts_cover_everything(world):
    for N in (333, 400, 500, 600, 777):
        cuts = H.dp_cuts(world, N)
        assert len(cuts) == world and cuts[0][0] == 0 and cuts[-1][1] == N
        assert all(cuts[r][1] == cuts[r + 1][0] for r in range(world - 1))
        sizes = [hi - lo for lo, hi in cuts]
        assert min(sizes) == 1 and sum(sizes) == N
        assert sizes[:-1] == list(H.DP_CUT_HEADS[world]) and sizes[-1] == N - sum(H.DP_CUT_HEADS[world])
    assert {15, 16, 17} <= set(H.DP_CUT_HEADS[8]) and 17 in H.DP_CUT_HEADS[3]          # one below, at and one above the 16-point tile
    with pytest.raises(AssertionError):
        H.dp_cuts(world, sum(H.DP_CUT_HEADS[world]))                                    # no points left for the last rank


def test_param_blocks_partition_the_flat_vector():
    for layers, kind in (([2, 64, 64, 1], go.NET_MLP), ([1, 64, 64, 64, 1], go.NET_RESIDUAL), ([3, 100, 100, 2], go.NET_MLP)):
        blocks = H.param_blocks(layers, kind)
        allidx = np.concatenate([ix for _, ix in blocks])
        assert np.array_equal(np.sort(allidx), np.arange(go.param_count(layers, kind)))
        assert len(blocks) == 2 * (len(go.expand_layers(layers, kind)[0]) - 1)


def test_float32_oracle_accumulates_the_gradient_over_the_points_in_float64():
    """the oracle on float32 inputs keeps float64 accumulators for every sum over the points, dW / db of mlp_backward included: with
    float32 ones, np.einsum's one-after-the-other sum lost 1.5e-5 of max|dW| of the output map on this case (the GPU matrix asks the
    float32 call for 1e-5 per block, to show that the engine's 5e-5 is within reach of fp32 arithmetic)"""
    kw = CASES["3d_energy_lambda_p5_256x2"][0]
    N = 400
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    pb = go.Problem(**kw, n_global=N)
    _, g64, _ = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64))
    _, g32, _ = go.full_loss_and_grad(pb, flat, x, x_bc)
    errs = H.block_rel_errs(g32, g64, H.param_blocks(pb.layers, pb.net_kind))
    assert max(errs.values()) < 1e-5, errs


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", ADDITIVE)
def test_oracle_is_additive_over_the_explicit_cuts(name, world):
    kw, N, _ = CASES[name]
    x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
    x, flat, x_bc = x.astype(np.float64), flat.astype(np.float64), x_bc.astype(np.float64)
    pb = go.Problem(**kw, n_global=N)
    if name == "2d_class_loss_64x4":
        assert pb.lambda_kind == go.LAMBDA_ENERGY and pb.w_reg_f != 0.0 and pb.w_reg_lam != 0.0
    ref, gref, _ = go.full_loss_and_grad(pb, flat, x, x_bc)
    cuts = H.dp_cuts(world, N)
    parts = [go.loss_and_grad(pb, flat, x[lo:hi], phase=1) for lo, hi in cuts]
    tot = {k: 0.0 for k in parts[0]}
    for p in parts:                                    # rank order
        for k in tot:
            tot[k] += p[k]
    res = [go.loss_and_grad(pb, flat, x[lo:hi], x_bc, shard_sums=tot) for lo, hi in cuts]          # the boundary batch is replicated
    grad = np.zeros_like(gref)
    sr2 = 0.0
    for r in res:
        grad += r["grad_local"] + r["grad_bc"] / world
        sr2 += r["sum_r2"]
    for r in res:                                      # every rank assembles the same scalars
        sc = go.assemble(pb, r, sum_r2_total=sr2, n_global=N)
        for k in ref:
            assert abs(sc[k] - ref[k]) <= 1e-12 * abs(ref[k]), (k, sc[k], ref[k])
    assert H.rel_err(grad, gref) < 1e-12
    worst = H.block_rel_errs(grad, gref, H.param_blocks(pb.layers, pb.net_kind))
    assert max(worst.values()) < 1e-12, worst
