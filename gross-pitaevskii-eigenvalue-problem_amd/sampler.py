"""The engine's stratified collocation sets, restated in numpy (csrc/gpe_sampler.h, include/gpe_hip.h: gpe_bind_sampler).

A set is a pure function of (seed, draw, cell): one uniformly placed point per cell of a regular grid, the random words from
Philox4x32-10 with the cell and the draw as counter and the seed as key.  `stratified_points` gives, bit for bit, what
`Engine.bind_sampler` holds on the device, so any training set of a run can be rebuilt on the CPU -- on any rank layout: cells are
numbered row-major (last axis fastest, the order of ``np.meshgrid(..., indexing="ij")`` ravelled) and a rank's batch is a contiguous
block of them.

The coordinate arithmetic is pinned: u = float32(r >> 8) * 2^-24 (exact), t = float32(i) + u (one rounded fp32 add),
x = lo + t * h (one rounded fp32 multiply, one rounded fp32 add -- never an fma), h = float32((double(hi) - double(lo)) / cells),
then the clip box by comparisons.  numpy's float32 array arithmetic rounds after every operation, which is exactly that.
"""
from __future__ import annotations

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., SC'11).  counter [..., 4], key [..., 2] (uint32 words, broadcast against each other) -> the four
    output words [..., 4] as uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    if c.shape[-1] != 4 or k.shape[-1] != 2:
        raise ValueError("philox4x32: counter is [..., 4] words, key [..., 2]")
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead).copy() for i in range(2))
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    w0, w1 = np.uint64(PHILOX_W0), np.uint64(PHILOX_W1)
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + w0) & _MASK, (k1 + w1) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _per_axis(v, d, name):
    a = np.asarray(v, dtype=np.float32).ravel()
    if a.size == 1:
        a = np.repeat(a, d)
    if a.size != d:
        raise ValueError(f"{name}: one value or one per axis ({d})")
    return a


def grid_spec(lo, hi, shape, clip=None):
    """(shape int64 [d], lo, hi, h, clip_lo, clip_hi as float32 [d]) -- the numbers the engine's kernel is given."""
    shape = np.atleast_1d(np.asarray(shape, dtype=np.int64))
    d = shape.size
    if not 1 <= d <= 3 or np.any(shape <= 0) or np.any(shape > 1 << 24):
        raise ValueError("shape: 1 to 3 axes of 1 .. 2^24 cells")
    lo, hi = _per_axis(lo, d, "lo"), _per_axis(hi, d, "hi")
    if np.any(hi <= lo):
        raise ValueError("hi <= lo")
    clo, chi = (lo, hi) if clip is None else (_per_axis(clip[0], d, "clip[0]"), _per_axis(clip[1], d, "clip[1]"))
    if np.any(chi < clo):
        raise ValueError("clip[1] < clip[0]")
    h = ((hi.astype(np.float64) - lo.astype(np.float64)) / shape).astype(np.float32)
    return shape, lo, hi, h, clo, chi


def stratified_points(lo, hi, shape, seed, draw, first_cell: int = 0, n=None, clip=None) -> np.ndarray:
    """Draw `draw` of the stratified set with seed `seed`: rows are cells first_cell .. first_cell + n - 1 (n None: all cells) of the
    grid of `shape` cells over [lo, hi]; clip = (clip_lo, clip_hi), default (lo, hi).  float32 [n, d]."""
    shape, lo, hi, h, clo, chi = grid_spec(lo, hi, shape, clip)
    d = shape.size
    total = int(np.prod([int(s) for s in shape]))
    first_cell = int(first_cell)
    n = total - first_cell if n is None else int(n)
    if first_cell < 0 or n <= 0 or first_cell + n > total:
        raise ValueError(f"cells [{first_cell}, {first_cell + n}) outside the grid's {total}")
    return _uniform_rows(np.arange(first_cell, first_cell + n, dtype=np.uint64), shape, lo, h, clo, chi, seed, draw)


def _words(cell, seed, draw):
    """The four Philox words of every cell (uint64 [n]) of draw `draw`: counter (cell lo, cell hi, draw lo, draw hi), key (seed lo, seed hi)."""
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    ctr = np.empty((cell.size, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = cell & _MASK, cell >> _S32
    ctr[:, 2], ctr[:, 3] = draw & 0xFFFFFFFF, draw >> 32
    return philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))


def _uniform_rows(cell, shape, lo, h, clo, chi, seed, draw):
    """One row per entry of `cell` (uint64 row-major indices of the grid, any order, any subset): stratified_points and cells_points."""
    d = shape.size
    r = _words(cell, seed, draw)
    idx = np.unravel_index(cell.astype(np.int64), tuple(int(s) for s in shape))          # row-major: last axis fastest
    x = np.empty((cell.size, d), dtype=np.float32)
    for k in range(d):
        u = (r[:, k] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        t = idx[k].astype(np.float32) + u
        xk = lo[k] + t * h[k]
        xk = np.where(xk < clo[k], clo[k], xk)
        xk = np.where(xk > chi[k], chi[k], xk)
        x[:, k] = xk
    return x


def node_centred(half, n_nodes):
    """(lo, hi, clip) whose cells are centred on the n_nodes nodes of the endpoint grid linspace(-half, half, n_nodes) per axis, with
    the physical box as clip box: what tools/accuracy_nd.py and tools/accuracy_cfg4.py train on."""
    half = np.atleast_1d(np.asarray(half, dtype=np.float64))
    n_nodes = np.atleast_1d(np.asarray(n_nodes, dtype=np.int64))
    hh = 2.0 * half / (n_nodes - 1)
    return -half - hh / 2, half + hh / 2, (-half, half)


# ---- graded grids (csrc/gpe_sampler.h: k_sampler_draw_graded, include/gpe_hip.h: gpe_bind_sampler_graded) -----------------------------
# The same draw on a tensor-product grid with caller-given, non-uniform cell edges; every point is weighted by its cell's volume.  Per
# axis, cell i: a = edges[i], b = edges[i + 1], w = b - a (one rounded fp32 subtraction), x = a + u * w (one rounded multiply, one
# rounded add), the clip by comparisons; weight q = w_0, then q * w_1, then * w_2 (rounded fp32 multiplies in axis order); total
# W = product over the axes of the fp64 sums, in index order, of the fp32 widths.

def _edges(edges):
    """[float32 array of cell edges per axis]; a single 1D array of numbers is one axis."""
    if isinstance(edges, np.ndarray) and edges.ndim == 1 or (len(edges) > 0 and np.isscalar(edges[0])):
        edges = [edges]
    ed = [np.ascontiguousarray(np.asarray(a, dtype=np.float32).ravel()) for a in edges]
    if not 1 <= len(ed) <= 3:
        raise ValueError("edges: 1 to 3 axes")
    for a in ed:
        if a.size < 2 or a.size - 1 > 1 << 24 or not np.all(np.isfinite(a)) or not np.all(a[1:] > a[:-1]):
            raise ValueError("edges: per axis 2 .. 2^24 + 1 finite, strictly increasing values")
    return ed


def _graded_block(ed, first_cell, n):
    shape = tuple(a.size - 1 for a in ed)
    total = int(np.prod([int(s) for s in shape]))
    first_cell = int(first_cell)
    n = total - first_cell if n is None else int(n)
    if first_cell < 0 or n <= 0 or first_cell + n > total:
        raise ValueError(f"cells [{first_cell}, {first_cell + n}) outside the grid's {total}")
    cell = np.arange(first_cell, first_cell + n, dtype=np.uint64)
    return cell, np.unravel_index(cell.astype(np.int64), shape)          # row-major: last axis fastest


def graded_points(edges, seed, draw, first_cell: int = 0, n=None, clip=None) -> np.ndarray:
    """Draw `draw` of the graded stratified set with seed `seed`: rows are cells first_cell .. first_cell + n - 1 (n None: all cells) of
    the grid bounded by `edges`; clip = (clip_lo, clip_hi), default the end edges.  float32 [n, d]: what Engine.bind_sampler_graded holds."""
    ed = _edges(edges)
    d = len(ed)
    cell, idx = _graded_block(ed, first_cell, n)
    clo = np.array([a[0] for a in ed], np.float32) if clip is None else _per_axis(clip[0], d, "clip[0]")
    chi = np.array([a[-1] for a in ed], np.float32) if clip is None else _per_axis(clip[1], d, "clip[1]")
    if np.any(chi < clo):
        raise ValueError("clip[1] < clip[0]")
    return _graded_rows(ed, cell, idx, clo, chi, seed, draw)


def _graded_rows(ed, cell, idx, clo, chi, seed, draw):
    """One row per entry of `cell` (uint64, with its per-axis indices idx): graded_points and cells_points."""
    d = len(ed)
    r = _words(cell, seed, draw)
    x = np.empty((cell.size, d), dtype=np.float32)
    for k in range(d):
        u = (r[:, k] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        a, b = ed[k][idx[k]], ed[k][idx[k] + 1]
        w = b - a
        xk = a + u * w
        xk = np.where(xk < clo[k], clo[k], xk)
        xk = np.where(xk > chi[k], chi[k], xk)
        x[:, k] = xk
    return x


def graded_weights(edges, first_cell: int = 0, n=None) -> np.ndarray:
    """The cell volumes of rows first_cell .. first_cell + n - 1, float32 [n]: the weights Engine.bind_sampler_graded binds (no draw
    changes them)."""
    ed = _edges(edges)
    _, idx = _graded_block(ed, first_cell, n)
    q = None
    for k in range(len(ed)):
        w = ed[k][idx[k] + 1] - ed[k][idx[k]]
        q = w if q is None else q * w
    return q.astype(np.float32)


def graded_total(edges) -> float:
    """W of the whole grid as the engine forms it: per axis the fp64 sum, in index order, of the fp32 widths; their product in axis order."""
    W = 1.0
    for a in _edges(edges):
        w = (a[1:] - a[:-1]).astype(np.float64)
        W *= float(np.cumsum(w)[-1])                  # (cumsum adds in index order; np.sum adds pairwise)
    return W


def sinh_edges(half, cells, stretch):
    """cells + 1 edges on [-half, half], refined towards the centre: x_i = half * sinh(stretch * t_i) / sinh(stretch), t_i = -1 + 2 i / cells
    (centre cells are narrower than the outer ones by about stretch / sinh(stretch) ... stretch * cosh(stretch) / sinh(stretch)).
    stretch -> 0 gives the uniform grid.  Symmetric by construction, end edges exactly -half and half.  float32."""
    cells = int(cells)
    if cells < 1 or not half > 0 or stretch < 0:
        raise ValueError("sinh_edges: cells >= 1, half > 0, stretch >= 0")
    t = (2.0 * np.arange(cells + 1, dtype=np.float64) - cells) / cells          # exactly antisymmetric: t[cells - i] == -t[i]
    r = np.abs(t) if stretch < 1e-8 else np.sinh(stretch * np.abs(t)) / np.sinh(stretch)
    e = (half * r).astype(np.float32) * np.sign(t).astype(np.float32)
    e[0], e[-1] = -np.float32(half), np.float32(half)
    return e


# ---- a subset of the cells (csrc/gpe_sampler.h: k_sampler_draw_cells / k_sampler_draw_graded_cells, include/gpe_hip.h: gpe_sampler_cells) ----
# Row j of the set is cell cells[j] of the grid, everything else as above: cells_points is stratified_points(...)[cells] (edges None) or
# graded_points(...)[cells], computed from the listed cells alone -- the same helper functions on another index array -- so a grid far too
# large to build is fine.  The weights of the graded form are the listed cells' volumes, their total W the fp64 sum in list order.

def _cell_list(cells, shape):
    c = np.asarray(cells)
    if c.size and not np.issubdtype(c.dtype, np.integer):
        raise ValueError("cells: integers")
    c = c.astype(np.int64).ravel()
    total = 1
    for s in shape:
        total *= int(s)
    if c.size and (int(c.min()) < 0 or int(c.max()) >= total):
        raise ValueError(f"cells: outside the grid's {total}")
    if np.any(c[1:] <= c[:-1]):
        raise ValueError(f"cells: not strictly ascending at position {int(np.flatnonzero(c[1:] <= c[:-1])[0]) + 1}")
    return c


def cells_points(cells, lo, hi, shape, seed, draw, clip=None, edges=None) -> np.ndarray:
    """Draw `draw` of the set Engine.bind_sampler_cells holds with the whole list: float32 [len(cells), d], row j the point of cell
    cells[j].  edges None: the uniform grid of `shape` cells over [lo, hi]; else the graded grid bounded by `edges` (lo, hi are its end
    edges and are not read).  clip as for stratified_points / graded_points.  A block of rows is a slice of the result."""
    if edges is None:
        shape, lo, hi, h, clo, chi = grid_spec(lo, hi, shape, clip)
        c = _cell_list(cells, shape)
        return _uniform_rows(c.astype(np.uint64), shape, lo, h, clo, chi, seed, draw)
    ed = _edges(edges)
    d = len(ed)
    shp = tuple(a.size - 1 for a in ed)
    if tuple(int(s) for s in np.atleast_1d(np.asarray(shape)).ravel()) != shp:
        raise ValueError("edges: shape[k] + 1 values per axis")
    c = _cell_list(cells, shp)
    clo = np.array([a[0] for a in ed], np.float32) if clip is None else _per_axis(clip[0], d, "clip[0]")
    chi = np.array([a[-1] for a in ed], np.float32) if clip is None else _per_axis(clip[1], d, "clip[1]")
    if np.any(chi < clo):
        raise ValueError("clip[1] < clip[0]")
    return _graded_rows(ed, c.astype(np.uint64), np.unravel_index(c, shp), clo, chi, seed, draw)


def cells_weights(cells, edges) -> np.ndarray:
    """The volumes of the listed cells, float32 [len(cells)]: graded_weights(edges)[cells], from the listed cells alone."""
    ed = _edges(edges)
    shp = tuple(a.size - 1 for a in ed)
    idx = np.unravel_index(_cell_list(cells, shp), shp)
    q = None
    for k in range(len(ed)):
        w = ed[k][idx[k] + 1] - ed[k][idx[k]]
        q = w if q is None else q * w
    return q.astype(np.float32)


def cells_total(cells, edges) -> float:
    """W of the graded cell-subset sampler: the fp64 sum, in list order, of cells_weights (0.0 for an empty list)."""
    q = cells_weights(cells, edges).astype(np.float64)
    return float(np.cumsum(q)[-1]) if q.size else 0.0          # (cumsum adds in list order; np.sum adds pairwise)


def cell_centres(lo, hi, shape, edges=None):
    """[float64 array of cell centres per axis].  Uniform grid: ((shape - i - 1/2) lo + (i + 1/2) hi) / shape with lo, hi as the engine
    holds them (rounded to float32 first) -- a form that maps i -> shape - 1 - i onto c -> -c exactly when lo = -hi; graded: the
    midpoints of the float32 edges."""
    if edges is not None:
        return [(a[:-1].astype(np.float64) + a[1:].astype(np.float64)) / 2 for a in _edges(edges)]
    shape, lo, hi, _, _, _ = grid_spec(lo, hi, shape)
    out = []
    for k in range(shape.size):
        i = np.arange(int(shape[k]), dtype=np.float64)
        out.append(((float(shape[k]) - i - 0.5) * float(lo[k]) + (i + 0.5) * float(hi[k])) / float(shape[k]))
    return out


def mask_cells(lo, hi, shape, predicate, edges=None) -> np.ndarray:
    """The cells whose centre satisfies `predicate` -- called with a float64 [n, d] array of centres, returning n booleans -- as the
    ascending int64 list bind_sampler_cells takes.  Host-only; the grid is walked in slabs along its first axis, never built whole."""
    cen = cell_centres(lo, hi, shape, edges)
    shp = [a.size for a in cen]
    d = len(shp)
    rest = np.stack([g.ravel() for g in np.meshgrid(*cen[1:], indexing="ij")], axis=1) if d > 1 else np.zeros((1, 0))
    out = []
    for i in range(shp[0]):
        x = np.concatenate([np.full((rest.shape[0], 1), cen[0][i]), rest], axis=1)
        keep = np.asarray(predicate(x), dtype=bool).ravel()
        if keep.size != rest.shape[0]:
            raise ValueError("predicate: one boolean per centre")
        out.append(np.flatnonzero(keep).astype(np.int64) + i * rest.shape[0])
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def ball_cells(lo, hi, shape, radius, centre=None, edges=None) -> np.ndarray:
    """The cells whose CENTRE lies within `radius` of `centre` (default the origin): sum_k (c_k - centre_k)^2 <= radius^2 in float64,
    the squares added in axis order.  An interval, a disk or a ball by the grid's dimension; ascending int64.  radius <= 0 keeps nothing."""
    d = len(cell_centres(lo, hi, shape, edges))
    c0 = np.zeros(d) if centre is None else np.asarray(centre, dtype=np.float64).ravel()
    if c0.size != d:
        raise ValueError(f"centre: one value per axis ({d})")
    r2 = float(radius) ** 2

    def inside(x):
        s = np.zeros(x.shape[0])
        for k in range(d):
            s = s + (x[:, k] - c0[k]) ** 2
        return s <= r2 if radius > 0 else np.zeros(x.shape[0], dtype=bool)
    return mask_cells(lo, hi, shape, inside, edges)


# ---- residual-adaptive allocation (csrc/gpe_sampler.h: k_adaptive_alloc / k_sampler_draw_adaptive, include/gpe_hip.h: gpe_sampler_adaptive)
# The cells of a graded grid are BLOCKS that share N rows: block b holds rows [off_b, off_{b+1}), off the exclusive prefix sum of the
# counts.  The counts come from the block masses m_b (sum q r^2 of the PDE residual over the block's rows, formed on the device) and the
# block volumes v_b through two fp64 divisions per block and integers behind them, so Python's own integers restate them exactly:
#   ok = 0 < M < inf;  kA_b = ok ? floor(m_b / M * 2^30) : 0;  kV_b = floor(double(v_b) / V * 2^30);  k_b = (1024 - s) kA_b + s kV_b
#   K = exclusive prefix sum of k;  R = N - B n_min;  n_b = n_min + (K_{b+1} R) // K_B - (K_b R) // K_B
# Row j of block b has local index l = j - off_b; Philox counter (b, l, draw lo, draw hi) -- not the (cell lo, cell hi, ...) of the
# graded sampler: the two layouts meet only in local index 0 (so with one row per block the set equals graded_points) -- and weight float32(double(v_b) / n_b).

ADAPTIVE_MAX_POINTS = 1 << 22


def uniform_per_1024(share: float) -> int:
    """The share of the rows always allocated by volume, in (0, 1], as the engine's integer s = round(1024 * share) in [1, 1024]."""
    s = int(round(1024.0 * float(share)))
    if not 0.0 < float(share) <= 1.0 or not 1 <= s <= 1024:
        raise ValueError("uniform_share: in (0, 1], and at least 1 / 2048")
    return s


def adaptive_counts(mass, total, edges, n_points: int, n_min: int = 1, uniform_per_1024: int = 512) -> np.ndarray:
    """Rows per block, int32 [B]: mass float64 [B] and total as Engine.adaptive_state() reports them (mass None: the bind's allocation by
    volume, which is also what total = 0, NaN or inf gives), the blocks bounded by `edges`, n_points rows in all, at least n_min per
    block, uniform_per_1024 in [1, 1024] of 1024 parts allocated by volume.  Exact integer arithmetic behind two fp64 divisions per block."""
    v = graded_weights(edges).astype(np.float64)
    V = graded_total(edges)
    B, N, n_min, s = v.size, int(n_points), int(n_min), int(uniform_per_1024)
    if not 1 <= N <= ADAPTIVE_MAX_POINTS or n_min < 1 or B * n_min > N or not 1 <= s <= 1024:
        raise ValueError("adaptive_counts: 1 <= n_points <= 2^22, n_min >= 1, B * n_min <= n_points, 1 <= uniform_per_1024 <= 1024")
    M = 0.0 if mass is None else float(total)
    ok = M > 0.0 and M < np.inf
    kV = np.floor(v / V * 2.0 ** 30)
    kA = np.zeros(B)
    if mass is not None:
        m = np.asarray(mass, dtype=np.float64).ravel()
        if m.size != B:
            raise ValueError(f"adaptive_counts: one mass per block ({B})")
        ok = ok and bool(np.all(np.isfinite(m)))          # (the engine's total of masses with a NaN or inf among them is not finite)
        if ok:
            kA = np.floor(m / M * 2.0 ** 30)
    R = N - B * n_min
    K, ks = 0, []
    for a, b in zip(kA, kV):
        ks.append((1024 - s) * int(a) + s * int(b))          # Python integers from here on
    KB = sum(ks)
    if KB <= 0:
        raise ValueError("adaptive_counts: the volume shares all truncate to zero")
    assert KB * R < 2 ** 63
    out = np.empty(B, dtype=np.int32)
    for i, k in enumerate(ks):
        out[i] = n_min + ((K + k) * R) // KB - (K * R) // KB
        K += k
    return out


def _adaptive_rows(ed, counts):
    counts = np.asarray(counts, dtype=np.int64).ravel()
    shape = tuple(a.size - 1 for a in ed)
    if counts.size != int(np.prod([int(s) for s in shape])) or np.any(counts < 1):
        raise ValueError("counts: one count >= 1 per block")
    b = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    l = np.arange(b.size, dtype=np.int64) - off[b]
    return counts, b, l, np.unravel_index(b, shape)


def adaptive_points(edges, counts, seed, draw, clip=None) -> np.ndarray:
    """Draw `draw` of the adaptive set with seed `seed` and `counts` rows per block: float32 [sum(counts), d], what
    Engine.bind_sampler_adaptive holds while adaptive_state()['counts'] == counts."""
    ed = _edges(edges)
    d = len(ed)
    counts, b, l, idx = _adaptive_rows(ed, counts)
    clo = np.array([a[0] for a in ed], np.float32) if clip is None else _per_axis(clip[0], d, "clip[0]")
    chi = np.array([a[-1] for a in ed], np.float32) if clip is None else _per_axis(clip[1], d, "clip[1]")
    if np.any(chi < clo):
        raise ValueError("clip[1] < clip[0]")
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    ctr = np.empty((b.size, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = b.astype(np.uint64), l.astype(np.uint64)
    ctr[:, 2], ctr[:, 3] = draw & 0xFFFFFFFF, draw >> 32
    r = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    x = np.empty((b.size, d), dtype=np.float32)
    for k in range(d):
        u = (r[:, k] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        lo, hi = ed[k][idx[k]], ed[k][idx[k] + 1]
        w = hi - lo
        xk = lo + u * w
        xk = np.where(xk < clo[k], clo[k], xk)
        xk = np.where(xk > chi[k], chi[k], xk)
        x[:, k] = xk
    return x


def adaptive_weights(edges, counts) -> np.ndarray:
    """float32 [sum(counts)]: every row of block b weighs float32(double(v_b) / n_b) -- one fp64 division, one conversion."""
    ed = _edges(edges)
    counts, b, _, _ = _adaptive_rows(ed, counts)
    q = graded_weights(ed).astype(np.float64) / counts.astype(np.float64)
    return q.astype(np.float32)[b]
