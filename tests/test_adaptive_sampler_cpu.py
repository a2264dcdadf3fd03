"""The numpy / Python-integer restatement of the residual-adaptive sampler (gpe_pinn.sampler: adaptive_counts, adaptive_points,
adaptive_weights) held to the arithmetic include/gpe_hip.h states for gpe_sampler_adaptive, and the two entry points in the ctypes
table.  tests/test_gpu_adaptive_sampler.py holds the device to this restatement."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from gpe_pinn import capi
from gpe_pinn import sampler as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {
    "1d": [S.sinh_edges(6.0, 8, 2.0)],
    "2d": [S.sinh_edges(4.0, 5, 1.5), np.linspace(-3, 3, 5).astype(np.float32)],
    "3d": [S.sinh_edges(4.0, 3, 1.5), S.sinh_edges(3.0, 4, 2.0), np.linspace(-2, 2, 6).astype(np.float32)],
}
PARAMS = [("1d", 256, 1, 256), ("2d", 1000, 2, 256), ("2d", 1000, 50, 1), ("3d", 777, 3, 1000), ("3d", 60, 1, 512)]


def masses(B, seed=0):
    return np.random.default_rng(seed).random(B) ** 4 * 3.7


def total(m):
    return float(np.cumsum(m)[-1])


def shares(m, M, ed, s):
    """k_b in Python integers, from the two fp64 divisions the header states"""
    v = S.graded_weights(ed).astype(np.float64)
    V = S.graded_total(ed)
    ok = M > 0 and np.isfinite(M)
    return [(1024 - s) * (int(np.floor(a / M * 2.0 ** 30)) if ok else 0) + s * int(np.floor(b / V * 2.0 ** 30)) for a, b in zip(m, v)]


@pytest.mark.parametrize("grid,N,n_min,s", PARAMS)
def test_counts_add_up_keep_the_minimum_and_stay_within_one_of_their_share(grid, N, n_min, s):
    ed = GRIDS[grid]
    B = S.graded_weights(ed).size
    m = masses(B)
    c = S.adaptive_counts(m, total(m), ed, N, n_min, s)
    assert c.dtype == np.int32 and c.shape == (B,) and int(c.sum()) == N and c.min() >= n_min
    k = shares(m, total(m), ed, s)
    R, KB = N - B * n_min, sum(k)
    for b in range(B):
        assert abs(Fraction(int(c[b]) - n_min) - Fraction(R * k[b], KB)) < 1          # exact rationals: no rounding in the check itself
    # ... and they are the stated formula, term by term
    K = np.concatenate([[0], np.cumsum(np.array(k, dtype=object))])
    assert [int(x) for x in c] == [n_min + (int(K[b + 1]) * R) // KB - (int(K[b]) * R) // KB for b in range(B)]


@pytest.mark.parametrize("grid,N,n_min,s", [p for p in PARAMS if p[1] > 20 * p[2] + 100])          # (cases with spare rows to move)
def test_every_fallback_gives_the_allocation_by_volume(grid, N, n_min, s):
    ed = GRIDS[grid]
    B = S.graded_weights(ed).size
    m = masses(B)
    vol = S.adaptive_counts(None, 0.0, ed, N, n_min, s)
    assert np.array_equal(S.adaptive_counts(m, 0.0, ed, N, n_min, s), vol)
    for bad in (np.nan, np.inf):
        mb = m.copy(); mb[B // 2] = bad
        with np.errstate(invalid="ignore"):
            assert np.array_equal(S.adaptive_counts(mb, float(np.cumsum(mb)[-1]), ed, N, n_min, s), vol)          # the total the device would form
        assert np.array_equal(S.adaptive_counts(mb, total(m), ed, N, n_min, s), vol)
        assert np.array_equal(S.adaptive_counts(m, bad, ed, N, n_min, s), vol)
    # s = 1024: the masses have no say, whatever they are; and the volume allocation follows the volumes
    assert np.array_equal(S.adaptive_counts(m, total(m), ed, N, n_min, 1024), S.adaptive_counts(None, 0.0, ed, N, n_min, 1024))
    v = S.graded_weights(ed).astype(np.float64)
    assert np.all(np.abs(vol - n_min - (N - B * n_min) * v / S.graded_total(ed)) < 1 + 1e-3)
    assert not np.array_equal(S.adaptive_counts(m, total(m), ed, N, n_min, s), vol)          # (the masses do have a say below 1024)


def test_counts_do_not_change_when_all_masses_are_scaled_by_a_power_of_two():
    ed = GRIDS["2d"]
    m = masses(20, seed=3)
    ref = S.adaptive_counts(m, total(m), ed, 1000, 2, 256)
    for e in (-600, -40, -1, 1, 17, 500):          # (m / M is the same quotient: scaling by 2^e is exact on both, far from under- and overflow)
        ms = np.ldexp(m, e)
        assert total(ms) == np.ldexp(total(m), e)
        assert np.array_equal(S.adaptive_counts(ms, total(ms), ed, 1000, 2, 256), ref)


@pytest.mark.parametrize("s", [1, 256, 1000])
def test_all_mass_in_one_block_gives_it_everything_but_the_volume_share_of_the_rest(s):
    ed, N, n_min = GRIDS["2d"], 1000, 2
    v = S.graded_weights(ed).astype(np.float64)
    B, V = v.size, S.graded_total(ed)
    R = N - B * n_min
    for hot in (0, 7, B - 1):
        m = np.zeros(B); m[hot] = 0.3
        c = S.adaptive_counts(m, 0.3, ed, N, n_min, s)
        rest = R * (s / 1024.0) * (V - v[hot]) / V
        assert abs(int(c[hot]) - (n_min + R - rest)) <= B, (s, hot, c[hot], n_min + R - rest)


def test_the_largest_accepted_sizes_stay_in_64_bits_and_match_big_integers():
    """N = 2^22 with a steep mass profile on 2^10 blocks, and B * n_min = N (no spare row: every count is n_min).  Every intermediate of
    the device's unsigned 64-bit arithmetic -- K_B R and below -- is formed here in Python integers and must stay below 2^63."""
    ed = [S.sinh_edges(5.0, 32, 3.0), S.sinh_edges(5.0, 32, 1.0)]
    B, N = 1024, 1 << 22
    m = masses(B, seed=9) * np.exp(np.linspace(0, 30, B))
    for s, n_min in ((1, 1), (1024, 1), (512, 4095), (512, 4096)):
        k = shares(m, total(m), ed, s)
        R, KB = N - B * n_min, sum(k)
        assert 0 < KB <= 1024 * 2 ** 30 + 1024 and KB * R < 2 ** 63
        c = S.adaptive_counts(m, total(m), ed, N, n_min, s)
        K, want = 0, []
        for kb in k:
            want.append(n_min + ((K + kb) * R) // KB - (K * R) // KB)
            K += kb
        assert [int(x) for x in c] == want and int(c.sum()) == N
        if n_min == 4096:
            assert R == 0 and (c == 4096).all()
    with pytest.raises(ValueError):
        S.adaptive_counts(m, total(m), ed, N + 1, 1, 512)
    with pytest.raises(ValueError):
        S.adaptive_counts(m, total(m), ed, N, 4097, 512)
    for bad_s in (0, 1025):
        with pytest.raises(ValueError):
            S.adaptive_counts(m, total(m), ed, N, 1, bad_s)
    # one block per row, the most blocks a bind accepts at this N
    ed1 = [np.linspace(-1, 1, (1 << 16) + 1).astype(np.float32)]
    c = S.adaptive_counts(None, 0.0, ed1, 1 << 16, 1, 512)
    assert (c == 1).all()


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_points_lie_inside_their_block_and_the_clip_box(grid):
    ed = GRIDS[grid]
    d = len(ed)
    shape = tuple(a.size - 1 for a in ed)
    B = int(np.prod(shape))
    m = masses(B, seed=1)
    c = S.adaptive_counts(m, total(m), ed, 40 * B + 13, 1, 128)
    x = S.adaptive_points(ed, c, seed=5, draw=2 ** 40 + 3)
    assert x.dtype == np.float32 and x.shape == (40 * B + 13, d)
    blk = np.repeat(np.arange(B), c)
    idx = np.unravel_index(blk, shape)                # row-major, last axis fastest
    for k in range(d):
        assert np.all(x[:, k] >= ed[k][idx[k]]) and np.all(x[:, k] <= ed[k][idx[k] + 1])
    clip = ([float(a[0]) * 0.8 for a in ed], [float(a[-1]) * 0.7 for a in ed])
    xc = S.adaptive_points(ed, c, seed=5, draw=2 ** 40 + 3, clip=clip)
    for k in range(d):
        lo, hi = np.float32(clip[0][k]), np.float32(clip[1][k])
        assert xc[:, k].min() >= lo and xc[:, k].max() <= hi
        inside = (x[:, k] >= lo) & (x[:, k] <= hi)
        assert np.array_equal(xc[inside, k], x[inside, k]) and np.all(np.isin(xc[~inside, k], [lo, hi]))
    # a pure function of (seed, draw, counts): another draw, another seed and other counts move the points
    assert np.array_equal(x, S.adaptive_points(ed, c, 5, 2 ** 40 + 3))
    assert not np.array_equal(x, S.adaptive_points(ed, c, 5, 2 ** 40 + 4)) and not np.array_equal(x, S.adaptive_points(ed, c, 6, 2 ** 40 + 3))


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_weights_of_a_block_add_up_to_its_volume(grid):
    ed = GRIDS[grid]
    v = S.graded_weights(ed).astype(np.float64)
    m = masses(v.size, seed=2)
    c = S.adaptive_counts(m, total(m), ed, 57 * v.size + 5, 1, 64)
    q = S.adaptive_weights(ed, c)
    assert q.dtype == np.float32 and q.shape == (int(c.sum()),)
    off = np.concatenate([[0], np.cumsum(c)])
    for b in range(v.size):
        rows = q[off[b]:off[b + 1]]
        assert (rows == np.float32(v[b] / float(c[b]))).all()                          # one fp64 division, one conversion
        assert abs(rows.sum(dtype=np.float64) - v[b]) <= int(c[b]) * 2.0 ** -24 * v[b]


def test_one_row_per_block_meets_the_graded_sampler_and_two_rows_do_not():
    """The Philox counter is (block, local index, draw lo, draw hi) here and (cell lo, cell hi, draw lo, draw hi) in the graded sampler.
    The layouts differ, so equality with graded_points is no promise of the interface -- but at one row per block (local index 0, block
    < 2^32) the two counters are the same four words, and the sets coincide; the asserts pin the layout by exactly that.  From the
    second row of a block on nothing matches."""
    ed = GRIDS["2d"]
    ones = np.ones(20, np.int32)
    assert np.array_equal(S.adaptive_weights(ed, ones), S.graded_weights(ed))
    a, g = S.adaptive_points(ed, ones, 11, 4), S.graded_points(ed, 11, 4)
    assert np.array_equal(a, g)                       # counter (b, 0, draw) == (cell, 0, draw)
    b = S.adaptive_points(ed, 2 * ones, 11, 4)
    assert np.array_equal(b[0::2], g)                 # local index 0 of every block is the same word whatever the counts ...
    assert not np.any(np.all(b[1::2] == g, axis=1))   # ... and local index 1 is another point of the same block, in every block


def test_share_mapping():
    assert S.uniform_per_1024(1.0) == 1024 and S.uniform_per_1024(0.25) == 256 and S.uniform_per_1024(1 / 1024) == 1
    for bad in (0.0, -0.1, 1.01, 1e-4):
        with pytest.raises(ValueError):
            S.uniform_per_1024(bad)


def test_entry_points_are_declared_and_bound_with_the_headers_arguments():
    hdr = open(os.path.join(ROOT, "include", "gpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    want = {"gpe_sampler_adaptive": ["gpe_engine*", "const gpe_sampler_spec*", "const float*", "const float*", "const float*", "int64_t", "int32_t", "int32_t"],
            "gpe_sampler_adaptive_state": ["gpe_engine*", "double*", "double*", "int32_t*", "int64_t*"],
            "gpe_sampler_adaptive_blocks": ["gpe_engine*", "int64_t*", "int64_t*"]}
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    table = {"gpe_sampler_adaptive": [vp, ctypes.POINTER(capi.gpe_sampler_spec), vp, vp, vp, i64, i32, i32],
             "gpe_sampler_adaptive_state": [vp, vp, ctypes.POINTER(ctypes.c_double), vp, ctypes.POINTER(i64)],
             "gpe_sampler_adaptive_blocks": [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]}
    for name, types in want.items():
        m = re.search(rf"^int\s+{name}\s*\(([^)]*)\)\s*;", code, re.M)
        assert m, name
        args = [" ".join(a.split()[:-1]) for a in m.group(1).split(",")]
        assert args == types, (name, args)
        res, argtypes = capi.SYMBOLS[name]
        assert res is ctypes.c_int and argtypes == table[name], name
    # the spec the bind takes is the graded sampler's, unchanged
    assert [n for n, _ in capi.gpe_sampler_spec._fields_] == ["shape", "lo", "hi", "clip_lo", "clip_hi", "seed", "first_cell", "n_local", "draw0", "every"]
    lib = ctypes.CDLL(capi.library_path())
    assert hasattr(lib, "gpe_sampler_adaptive") and hasattr(lib, "gpe_sampler_adaptive_state")
    lib.gpe_sizeof_sampler_spec.restype = ctypes.c_size_t
    assert lib.gpe_sizeof_sampler_spec() == ctypes.sizeof(capi.gpe_sampler_spec)
    # names chosen so that the live-engine table's patterns (gpe_bind_* / gpe_set_*) do not claim them
    assert not re.match(r"gpe_(bind|set)_", "gpe_sampler_adaptive")
