"""The cell-subset sampler's numpy restatement (gpe_pinn.sampler: cells_points, cells_weights, cells_total, ball_cells, mask_cells) held
to the full-grid restatements it indexes, and the two entry points (include/gpe_hip.h: gpe_sampler_cells, gpe_sampler_cells_read) in the
header, the library and the ctypes table.  Without a GPU gpe_create fails at its first HIP call (tests/test_create_refusals_cpu.py), so
the only refusal of the bind that is reachable here is the one of a missing engine; every other refusal needs a live engine and lives
in tests/test_gpu_sampler_cells.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gpe_pinn
from gpe_pinn import capi
from gpe_pinn import sampler as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, DRAW = 0xABCDEF0123456789, 2 ** 32 + 7          # both above 2^32: the high key word and the high draw word are not zero

# d: (lo, hi, shape, clip)
GRIDS = {1: ((-6.0,), (6.0,), (16,), None),
         2: ((-3.0, -2.5), (3.0, 2.5), (12, 10), ((-2.9, -2.4), (2.9, 2.4))),
         3: ((-3.0, -2.5, -2.0), (3.0, 2.5, 2.0), (6, 5, 4), None)}
EDGES = {1: [S.sinh_edges(6.0, 16, 2.0)], 2: [S.sinh_edges(3.0, 12, 2.5), S.sinh_edges(2.5, 10, 1.0)],
         3: [S.sinh_edges(3.0, 6, 1.5), S.sinh_edges(2.5, 5, 2.0), S.sinh_edges(2.0, 4, 0.5)]}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def lists(d):
    """the whole grid, a ball, every third cell, one cell, the last cell"""
    lo, hi, shape, _ = GRIDS[d]
    total = int(np.prod(shape))
    return [np.arange(total), S.ball_cells(lo, hi, shape, 2.0), np.arange(1, total, 3), np.array([total // 2]), np.array([total - 1])]


@pytest.mark.parametrize("d", [1, 2, 3])
def test_cells_points_is_the_full_restatement_indexed_by_the_list(d):
    lo, hi, shape, clip = GRIDS[d]
    full_u = S.stratified_points(lo, hi, shape, SEED, DRAW, clip=clip)
    full_g = S.graded_points(EDGES[d], SEED, DRAW, clip=clip)
    assert not np.array_equal(full_u, S.stratified_points(lo, hi, shape, SEED & 0xFFFFFFFF, DRAW, clip=clip))       # (the high words are read)
    assert not np.array_equal(full_u, S.stratified_points(lo, hi, shape, SEED, DRAW & 0xFFFFFFFF, clip=clip))
    for cells in lists(d):
        assert cells.size > 0
        u = S.cells_points(cells, lo, hi, shape, SEED, DRAW, clip=clip)
        g = S.cells_points(cells, lo, hi, shape, SEED, DRAW, clip=clip, edges=EDGES[d])
        assert u.dtype == g.dtype == np.float32 and u.shape == g.shape == (cells.size, d)
        assert np.array_equal(bits(u), bits(full_u[cells]))
        assert np.array_equal(bits(g), bits(full_g[cells]))


def test_a_grid_too_large_to_build_and_the_high_counter_word():
    """70 000 x 70 000 cells; the listed cells straddle 2^32, so counter word 1 is 0 for two of them and 1 for three"""
    n = 70000
    cells = np.array([0, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, n * n - 1], dtype=np.int64)
    lo, hi = (-4.0, -3.0), (4.0, 3.0)
    x = S.cells_points(cells, lo, hi, (n, n), SEED, DRAW)
    ctr = np.array([[c & 0xFFFFFFFF, c >> 32, DRAW & 0xFFFFFFFF, DRAW >> 32] for c in cells.tolist()], dtype=np.uint64)
    assert ctr[:, 1].tolist() == [0, 0, 1, 1, 1]
    r = S.philox4x32(ctr, np.array([SEED & 0xFFFFFFFF, SEED >> 32], dtype=np.uint64))
    for k in range(2):
        i = (cells // n if k == 0 else cells % n).astype(np.float32)
        h = np.float32((np.float64(np.float32(hi[k])) - np.float64(np.float32(lo[k]))) / n)
        u = (r[:, k] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        t = i + u
        want = np.float32(lo[k]) + t * h
        want = np.minimum(np.maximum(want, np.float32(lo[k])), np.float32(hi[k]))
        assert np.array_equal(bits(x[:, k]), bits(want)), k
    # the graded form on the same grid: uniform edges written out, the same five cells
    ed = [np.linspace(lo[k], hi[k], n + 1).astype(np.float32) for k in range(2)]
    g = S.cells_points(cells, lo, hi, (n, n), SEED, DRAW, edges=ed)
    q = S.cells_weights(cells, ed)
    for k in range(2):
        i = cells // n if k == 0 else cells % n
        a, b = ed[k][i], ed[k][i + 1]
        u = (r[:, k] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        assert np.array_equal(bits(g[:, k]), bits(a + u * (b - a))), k
    assert np.array_equal(bits(q), bits((ed[0][cells // n + 1] - ed[0][cells // n]) * (ed[1][cells % n + 1] - ed[1][cells % n])))


def test_ball_cells_on_the_disk_grid_is_the_brute_force_list():
    lo, hi, shape = (-3.0, -2.5), (3.0, 2.5), (12, 10)
    cells = S.ball_cells(lo, hi, shape, 2.0)
    want = []
    for i in range(12):
        for j in range(10):
            cx, cy = -3.0 + (i + 0.5) * 0.5, -2.5 + (j + 0.5) * 0.5          # (exact in binary: no centre lies on the circle)
            if cx * cx + cy * cy <= 4.0:
                want.append(i * 10 + j)
    assert cells.dtype == np.int64 and cells.tolist() == want and 40 < len(want) < 120
    assert np.all(np.diff(cells) > 0)
    mirrored = np.sort((11 - cells // 10) * 10 + cells % 10)                   # x -> -x
    assert np.array_equal(mirrored, cells)
    assert np.array_equal(np.sort(cells // 10 * 10 + (9 - cells % 10)), cells)          # y -> -y
    assert np.array_equal(S.ball_cells(lo, hi, shape, 100.0), np.arange(120))           # beyond the corners: every cell
    assert S.ball_cells(lo, hi, shape, 0.0).size == 0
    # an off-centre ball, and mask_cells with the same predicate
    off = S.ball_cells(lo, hi, shape, 1.0, centre=(1.0, -0.5))
    same = S.mask_cells(lo, hi, shape, lambda x: (x[:, 0] - 1.0) ** 2 + (x[:, 1] + 0.5) ** 2 <= 1.0)
    assert off.size > 0 and np.array_equal(off, same)
    half = S.mask_cells(lo, hi, shape, lambda x: x[:, 0] > 0)                  # a half-space cut
    assert np.array_equal(half, np.arange(60, 120))


@pytest.mark.parametrize("d", [1, 3])
def test_ball_cells_in_one_and_three_dimensions(d):
    lo, hi, shape, _ = GRIDS[d]
    cells = S.ball_cells(lo, hi, shape, 2.0)
    cen = S.cell_centres(lo, hi, shape)
    grid = np.stack([g.ravel() for g in np.meshgrid(*cen, indexing="ij")], axis=1)
    assert np.array_equal(cells, np.flatnonzero((grid ** 2).sum(1) <= 4.0))
    assert 0 < cells.size < grid.shape[0]


def test_the_bind_helper_raises_on_an_empty_list():
    class NoEngine(gpe_pinn.Engine):
        def __init__(self):                                                  # no library, no device: the helper must refuse before either
            pass

        def __del__(self):
            pass
    empty = S.ball_cells((-3.0, -2.5), (3.0, 2.5), (12, 10), 0.0)
    with pytest.raises(ValueError, match="empty"):
        NoEngine().bind_sampler_cells(empty, lo=(-3.0, -2.5), hi=(3.0, 2.5), shape=(12, 10), every=100)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_weights_and_total_of_the_list(d):
    ed = EDGES[d]
    full = S.graded_weights(ed)
    for cells in lists(d):
        q = S.cells_weights(cells, ed)
        assert q.dtype == np.float32 and np.array_equal(bits(q), bits(full[cells]))
        W = 0.0
        for v in full[cells]:
            W += float(v)                                                     # fp64, in list order
        assert S.cells_total(cells, ed) == W
    assert S.cells_total(np.zeros(0, np.int64), ed) == 0.0


def test_lists_the_restatement_refuses():
    lo, hi, shape, _ = GRIDS[2]
    for bad, text in (([3, 3], "position 1"), ([0, 5, 4, 9], "position 2"), ([-1, 2], "outside"), ([0, 120], "outside")):
        with pytest.raises(ValueError, match=text):
            S.cells_points(np.array(bad), lo, hi, shape, 1, 0)
        with pytest.raises(ValueError, match=text):
            S.cells_weights(np.array(bad), EDGES[2])
    with pytest.raises(ValueError):
        S.cells_points(np.array([0.5, 1.5]), lo, hi, shape, 1, 0)
    with pytest.raises(ValueError):
        S.cells_points(np.array([0, 1]), lo, hi, (12, 11), 1, 0, edges=EDGES[2])          # shape and edges disagree


def test_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "gpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"^int\s+gpe_sampler_cells\s*\(([^;]*)\)\s*;", code, re.M)
    assert m and [a.strip().rsplit(" ", 1)[0].strip() for a in m.group(1).split(",")] == \
        ["gpe_engine*", "const gpe_sampler_spec*", "const int64_t*", "int64_t", "const float*", "const float*", "const float*"]
    m = re.search(r"^int\s+gpe_sampler_cells_read\s*\(([^;]*)\)\s*;", code, re.M)
    assert m and [a.strip().rsplit(" ", 1)[0].strip() for a in m.group(1).split(",")] == \
        ["gpe_engine*", "const int64_t**", "int64_t*", "int64_t*"]
    assert not re.search(r"^int\s+gpe_bind_\w*cells", code, re.M)            # (tests/live_table.py holds every gpe_bind_* name)
    vp, i64 = C.c_void_p, C.c_int64
    assert capi.SYMBOLS["gpe_sampler_cells"] == (C.c_int, [vp, C.POINTER(capi.gpe_sampler_spec), vp, i64, vp, vp, vp])
    assert capi.SYMBOLS["gpe_sampler_cells_read"] == (C.c_int, [vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)])
    lib = capi.load()
    assert lib.gpe_sizeof_sampler_spec() == C.sizeof(capi.gpe_sampler_spec) == 112          # the spec keeps its size
    for name in ("bind_sampler_cells", "sampler_cells"):
        assert callable(getattr(gpe_pinn.Engine, name))


def test_a_missing_engine_is_refused_before_anything_is_read():
    lib = capi.load()
    sp = capi.gpe_sampler_spec()
    cells = np.arange(4, dtype=np.int64)
    assert lib.gpe_sampler_cells(None, C.byref(sp), cells.ctypes.data_as(C.c_void_p), 4, None, None, None) == capi.GPE_ERR_INVALID
    assert lib.gpe_sampler_cells(None, None, None, 0, None, None, None) == capi.GPE_ERR_INVALID
    n = C.c_int64(-5)
    assert lib.gpe_sampler_cells_read(None, None, C.byref(n), None) == capi.GPE_ERR_INVALID and n.value == -5
