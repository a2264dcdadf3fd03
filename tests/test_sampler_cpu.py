"""gpe_pinn.sampler on the CPU: the Philox4x32-10 known answers, and the stratified draw the engine's sampler is specified by
(include/gpe_hip.h: gpe_bind_sampler) -- cell order, cell membership, clip box, block invariance, reproducibility, uniformity -- plus
the layout of gpe_sampler_spec.  tests/test_gpu_sampler.py holds the device against stratified_points bit for bit."""
import ctypes

import numpy as np
import pytest

from gpe_pinn import capi
from gpe_pinn import sampler as S

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = S.philox4x32(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert tuple(int(v) for v in got) == want


def test_philox_is_vectorised_over_leading_axes():
    ctr = np.array([k[0] for k in KAT], dtype=np.uint32)
    key = np.array([k[1] for k in KAT], dtype=np.uint32)
    got = S.philox4x32(ctr, key)
    assert got.shape == (3, 4)
    assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in KAT]


GRIDS = {1: (dict(lo=-6.0, hi=6.0, shape=(300,))),
         2: (dict(lo=(-3.0, -2.5), hi=(3.0, 3.5), shape=(37, 41))),
         3: (dict(lo=(-3.0, -2.0, -1.5), hi=(3.0, 2.5, 1.0), shape=(11, 7, 13)))}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cell_bounds(lo, hi, shape):
    """closed interval of every row's cell per axis, in fp64, from the float32 lo / hi the draw is given"""
    shape = np.atleast_1d(np.asarray(shape, dtype=np.int64))
    d = shape.size
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float32), (d,)).astype(np.float64)
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float32), (d,)).astype(np.float64)
    h = ((hi - lo) / shape).astype(np.float32).astype(np.float64)      # the draw's h: float32((double(hi) - double(lo)) / cells)
    idx = np.stack(np.unravel_index(np.arange(int(np.prod(shape))), tuple(shape)), axis=1)      # row-major, last axis fastest
    return lo + idx * h, lo + (idx + 1) * h, idx, lo, hi


@pytest.mark.parametrize("d", [1, 2, 3])
def test_stratified_points_shape_order_and_cells(d):
    g = GRIDS[d]
    x = S.stratified_points(**g, seed=7, draw=3)
    a, b, idx, lo, hi = _cell_bounds(**g)
    n = int(np.prod(g["shape"]))
    assert x.dtype == np.float32 and x.shape == (n, d)
    # meshgrid(indexing="ij") ravelled is the same cell order
    axes = [np.arange(s) for s in g["shape"]]
    mesh = np.stack([m.ravel() for m in np.meshgrid(*axes, indexing="ij")], axis=1)
    assert np.array_equal(mesh, idx)
    for k in range(d):
        ulp = float(np.spacing(np.float32(max(abs(lo[k]), abs(hi[k])))))
        xk = x[:, k].astype(np.float64)
        assert np.all(xk >= a[:, k] - ulp) and np.all(xk <= b[:, k] + ulp), f"axis {k}: a point left its cell"
        assert np.all(x[:, k] >= np.float32(lo[k])) and np.all(x[:, k] <= np.float32(hi[k])), f"axis {k}: outside the clip box"


@pytest.mark.parametrize("d", [1, 2, 3])
def test_narrow_clip_box_holds(d):
    g = GRIDS[d]
    clip = (np.full(d, -1.0), np.full(d, 0.75))
    x = S.stratified_points(**g, seed=1, draw=0, clip=clip)
    assert x.min() >= np.float32(-1.0) and x.max() <= np.float32(0.75)
    free = S.stratified_points(**g, seed=1, draw=0)
    inside = (free >= np.float32(-1.0)) & (free <= np.float32(0.75))
    assert np.array_equal(_bits(x)[inside], _bits(free)[inside])          # the clip moves nothing that was inside


@pytest.mark.parametrize("d,half,nodes", [(1, 10.0, 257), (2, (6.0, 5.0), (64, 48)), (3, (4.0, 3.0, 2.5), (12, 10, 8))])
def test_node_centred_cells_stay_in_the_physical_box(d, half, nodes):
    lo, hi, clip = S.node_centred(half, nodes)
    half = np.atleast_1d(np.asarray(half, dtype=np.float64))
    nodes_a = np.atleast_1d(nodes)
    for draw in range(4):
        x = S.stratified_points(lo, hi, nodes_a, seed=11, draw=draw, clip=clip)
        assert x.shape == (int(np.prod(nodes_a)), d)
        grid = np.stack([m.ravel() for m in np.meshgrid(*[np.linspace(-half[k], half[k], nodes_a[k]) for k in range(d)], indexing="ij")], axis=1)
        hh = 2 * half / (nodes_a - 1)
        assert np.all(np.abs(x - grid) <= hh / 2 + 1e-5), "a point is not within half a cell of its node"
        for k in range(d):
            assert x[:, k].min() >= np.float32(-half[k]) and x[:, k].max() <= np.float32(half[k])      # first and last node's cells included
        first = x[idx_of_axis_extreme(nodes_a, 0)]
        last = x[idx_of_axis_extreme(nodes_a, 1)]
        assert np.all(first >= (-half).astype(np.float32)) and np.all(last <= half.astype(np.float32))


def idx_of_axis_extreme(nodes, which):
    """row of the cell with index 0 (which = 0) or shape - 1 (which = 1) on every axis"""
    return 0 if which == 0 else int(np.prod(nodes)) - 1


@pytest.mark.parametrize("d", [1, 2, 3])
def test_block_invariance(d):
    g = GRIDS[d]
    full = S.stratified_points(**g, seed=5, draw=9)
    n = full.shape[0]
    last = g["shape"][-1]
    cuts = [0, 1, last + 3 if last + 3 < n else 2, n // 2 + 1, n - 1, n]          # a split that is no multiple of the last axis among them
    assert any(c % last for c in cuts[1:-1]) or d == 1
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b <= a:
            continue
        part = S.stratified_points(**g, seed=5, draw=9, first_cell=a, n=b - a)
        assert np.array_equal(_bits(part), _bits(full[a:b])), (a, b)
    tail = S.stratified_points(**g, seed=5, draw=9, first_cell=n - 5)              # n None: all the remaining cells
    assert np.array_equal(_bits(tail), _bits(full[n - 5:]))


def test_same_seed_and_draw_repeat_others_differ():
    g = GRIDS[2]
    a = S.stratified_points(**g, seed=123456789012345, draw=2 ** 33 + 5)
    b = S.stratified_points(**g, seed=123456789012345, draw=2 ** 33 + 5)
    assert np.array_equal(_bits(a), _bits(b))
    for other in (dict(seed=123456789012346, draw=2 ** 33 + 5), dict(seed=123456789012345, draw=2 ** 33 + 6),
                  dict(seed=123456789012345, draw=5), dict(seed=123456789012345 + 2 ** 32, draw=2 ** 33 + 5)):
        c = S.stratified_points(**g, **other)
        assert np.mean(_bits(a) != _bits(c)) > 0.99, other


def test_uniform_inside_the_cells():
    """mean of (x - cell_lo)/h over 64 draws of a 64 x 64 grid: within 5 standard errors of 1/2 per axis (sigma of U(0,1) = 1/sqrt(12))"""
    g = dict(lo=(-8.0, -8.0), hi=(8.0, 8.0), shape=(64, 64))
    a, _, _, lo, hi = _cell_bounds(**g)
    h = ((hi - lo) / 64).astype(np.float32).astype(np.float64)
    frac = np.concatenate([(S.stratified_points(**g, seed=2024, draw=m).astype(np.float64) - a) / h for m in range(64)])
    n_samples = frac.shape[0]
    assert n_samples == 64 * 64 * 64
    bound = 5.0 / np.sqrt(12.0 * n_samples)
    for k in range(2):
        assert abs(frac[:, k].mean() - 0.5) <= bound, (k, frac[:, k].mean(), bound)


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        S.stratified_points(0.0, 0.0, (4,), 0, 0)
    with pytest.raises(ValueError):
        S.stratified_points(-1.0, 1.0, (4, 4), 0, 0, first_cell=10, n=7)
    with pytest.raises(ValueError):
        S.stratified_points(-1.0, 1.0, (4,), 0, 0, clip=(0.5, -0.5))


def test_sampler_spec_layout_matches_header():
    lib = ctypes.CDLL(capi.library_path())
    lib.gpe_sizeof_sampler_spec.restype = ctypes.c_size_t
    assert lib.gpe_sizeof_sampler_spec() == ctypes.sizeof(capi.gpe_sampler_spec)
    assert ctypes.sizeof(capi.gpe_sampler_spec) == 3 * 8 + 4 * 3 * 4 + 8 + 4 * 8
