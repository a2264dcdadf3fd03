// gpe_sampler.h -- stratified collocation sets drawn on the device (include/gpe_hip.h: gpe_bind_sampler).  One uniformly placed point
// per cell of a regular grid, from a counter-based generator, written in place into the engine's own point buffer.  Replaces the host
// loop of tools/accuracy_nd.py:run_epochs (16 jittered numpy copies of the grid, uploaded, cycled with gpe_bind_points); the reference
// has no counterpart: it trains on one fixed grid.
//
// The draw is a pure function of (seed, draw, cell) -- gpe_pinn/sampler.py restates it in numpy and the two agree bit for bit:
//   words  Philox4x32-10, counter (cell lo, cell hi, draw lo, draw hi), key (seed lo, seed hi); output word k serves axis k
//   u      float(r >> 8) * 2^-24                  exact: 24 bits
//   t      float(i_k) + u                         one rounded fp32 add (i_k < 2^24, checked at the bind)
//   x      lo[k] + t * h[k]                       one rounded multiply, one rounded add, never an fma: smp_mul_then_add below
//   clip   x < clip_lo ? clip_lo : x, then x > clip_hi ? clip_hi : x      (comparisons, not fmin/fmax: no choice between +0 and -0)
// Cells are numbered row-major, last axis fastest; row j of the buffer is cell first_cell + j, so contiguous blocks of cells held by
// different ranks are, together, the set one rank would hold.
// One thread per point, one Philox call per thread, plain vector stores (global_store_dword) only.
#pragma once
#include "gpe_common.h"

struct SamplerGrid {
    int64_t shape[3];
    float lo[3], h[3], clip_lo[3], clip_hi[3];
    uint32_t key0, key1;
    int dim;
};

#define SMP_THREADS 256

// lo + t * h in two roundings, whatever -ffp-contract the library is built with.  hipcc's default (fast-honor-pragmas) contracts the
// expression to an fma, and HIP's __fmul_rn / __fadd_rn are no protection: its headers define them as a plain `*` and `+`, which
// are contracted like any other.  The pragma takes the contract flag off the two operations; the empty asm makes the product opaque
// to the instruction selector, which under a forced -ffp-contract=fast fuses unflagged operations too.
GPE_DEV float smp_mul_then_add(float lo, float t, float h) {
#pragma clang fp contract(off)
    float p = t * h;
    asm volatile("" : "+v"(p));
    return lo + p;
}

GPE_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// x [n][dim] <- draw `draw` of cells [first_cell, first_cell + n);  xs (NULL: none) [2n][dim] <- [x ; -x], the symmetry batch
__global__ __launch_bounds__(SMP_THREADS) void k_sampler_draw(SamplerGrid g, int64_t first_cell, int64_t n, uint64_t draw,
                                                              float* __restrict__ x, float* __restrict__ xs) {
    const int64_t j = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (j >= n) return;
    const uint64_t cell = (uint64_t)(first_cell + j);
    uint32_t r[4];
    philox4x32_10((uint32_t)cell, (uint32_t)(cell >> 32), (uint32_t)draw, (uint32_t)(draw >> 32), g.key0, g.key1, r);
    uint64_t rest = cell;
    float v[3];
#pragma unroll
    for (int k = 2; k >= 0; --k) {
        if (k >= g.dim) continue;
        const uint64_t s = (uint64_t)g.shape[k];
        const uint64_t q = rest / s;
        const float ik = (float)(uint32_t)(rest - q * s);
        rest = q;
        const float u = (float)(r[k] >> 8) * 0x1p-24f;
        const float t = ik + u;
        float xv = smp_mul_then_add(g.lo[k], t, g.h[k]);
        xv = xv < g.clip_lo[k] ? g.clip_lo[k] : xv;
        xv = xv > g.clip_hi[k] ? g.clip_hi[k] : xv;
        v[k] = xv;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= g.dim) continue;
        x[j * g.dim + k] = v[k];
        if (xs) { xs[j * g.dim + k] = v[k]; xs[(n + j) * g.dim + k] = -v[k]; }
    }
}

// ---- graded grids (gpe_bind_sampler_graded) -------------------------------------------------------------------------------------------
// The same draw on a tensor-product grid with caller-given, non-uniform cell edges: axis k has shape[k] cells, cell i spans
// [edges_k[i], edges_k[i + 1]].  Same Philox call, counter / key layout, word per axis and cell numbering as k_sampler_draw; per axis
//   a, b   edges_k[i], edges_k[i + 1]
//   w      b - a                                  one rounded fp32 subtraction: the cell's width
//   x      a + u * w                              smp_mul_then_add: one rounded multiply, one rounded add, never an fma
//   clip   as above, by comparisons
// and the point's quadrature weight is its cell's volume q = w_0, then q * w_1, then * w_2: rounded fp32 multiplies in axis order.  The
// weights do not depend on the draw: qw != NULL (the bind) writes them, the redraws pass NULL.  g.lo / g.h are not read.
// gpe_pinn/sampler.py:graded_points / graded_weights restate both in numpy, bit for bit.  Plain vector stores only.
__global__ __launch_bounds__(SMP_THREADS) void k_sampler_draw_graded(SamplerGrid g, const float* __restrict__ e0, const float* __restrict__ e1,
                                                                     const float* __restrict__ e2, int64_t first_cell, int64_t n, uint64_t draw,
                                                                     float* __restrict__ x, float* __restrict__ qw) {
    const int64_t j = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (j >= n) return;
    const uint64_t cell = (uint64_t)(first_cell + j);
    uint32_t r[4];
    philox4x32_10((uint32_t)cell, (uint32_t)(cell >> 32), (uint32_t)draw, (uint32_t)(draw >> 32), g.key0, g.key1, r);
    uint64_t rest = cell;
    float v[3], w[3];
#pragma unroll
    for (int k = 2; k >= 0; --k) {
        if (k >= g.dim) continue;
        const float* __restrict__ ed = k == 0 ? e0 : (k == 1 ? e1 : e2);
        const uint64_t s = (uint64_t)g.shape[k];
        const uint64_t q = rest / s;
        const uint32_t ik = (uint32_t)(rest - q * s);         // < shape[k]: edges_k holds shape[k] + 1 entries
        rest = q;
        const float a = ed[ik], b = ed[ik + 1];
        const float u = (float)(r[k] >> 8) * 0x1p-24f;
        w[k] = b - a;
        float xv = smp_mul_then_add(a, u, w[k]);
        xv = xv < g.clip_lo[k] ? g.clip_lo[k] : xv;
        xv = xv > g.clip_hi[k] ? g.clip_hi[k] : xv;
        v[k] = xv;
    }
    float qv = w[0];
#pragma unroll
    for (int k = 1; k < 3; ++k) {
        if (k >= g.dim) continue;
        qv = qv * w[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= g.dim) continue;
        x[j * g.dim + k] = v[k];
    }
    if (qw) qw[j] = qv;
}

// ---- a subset of the cells (gpe_sampler_cells) ----------------------------------------------------------------------------------------
// The same two draws with one indirection: row j of the buffer is cell cells[first + j] of the grid instead of cell first_cell + j.
// `cells` is the engine-owned copy of the caller's strictly ascending list (a disk, a ball, any mask: gpe_pinn/sampler.py ball_cells /
// mask_cells); the bind checked every entry against [0, prod shape), so the per-axis index stays below shape[k] and the edge reads stay
// inside their arrays.  Everything behind the load is k_sampler_draw / k_sampler_draw_graded statement for statement, so row j holds the
// bits row cells[first + j] of the full grid's set holds: sampler.py cells_points is stratified_points(...)[cells] by construction.
// One thread per row; the 8-byte index loads of a wave are consecutive (one coalesced global_load_dwordx2 each); plain vector stores only.
__global__ __launch_bounds__(SMP_THREADS) void k_sampler_draw_cells(SamplerGrid g, const int64_t* __restrict__ cells, int64_t first, int64_t n,
                                                                    uint64_t draw, float* __restrict__ x, float* __restrict__ xs) {
    const int64_t j = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (j >= n) return;
    const uint64_t cell = (uint64_t)cells[first + j];
    uint32_t r[4];
    philox4x32_10((uint32_t)cell, (uint32_t)(cell >> 32), (uint32_t)draw, (uint32_t)(draw >> 32), g.key0, g.key1, r);
    uint64_t rest = cell;
    float v[3];
#pragma unroll
    for (int k = 2; k >= 0; --k) {
        if (k >= g.dim) continue;
        const uint64_t s = (uint64_t)g.shape[k];
        const uint64_t q = rest / s;
        const float ik = (float)(uint32_t)(rest - q * s);
        rest = q;
        const float u = (float)(r[k] >> 8) * 0x1p-24f;
        const float t = ik + u;
        float xv = smp_mul_then_add(g.lo[k], t, g.h[k]);
        xv = xv < g.clip_lo[k] ? g.clip_lo[k] : xv;
        xv = xv > g.clip_hi[k] ? g.clip_hi[k] : xv;
        v[k] = xv;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= g.dim) continue;
        x[j * g.dim + k] = v[k];
        if (xs) { xs[j * g.dim + k] = v[k]; xs[(n + j) * g.dim + k] = -v[k]; }
    }
}

__global__ __launch_bounds__(SMP_THREADS) void k_sampler_draw_graded_cells(SamplerGrid g, const float* __restrict__ e0, const float* __restrict__ e1,
                                                                           const float* __restrict__ e2, const int64_t* __restrict__ cells,
                                                                           int64_t first, int64_t n, uint64_t draw, float* __restrict__ x,
                                                                           float* __restrict__ qw) {
    const int64_t j = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (j >= n) return;
    const uint64_t cell = (uint64_t)cells[first + j];
    uint32_t r[4];
    philox4x32_10((uint32_t)cell, (uint32_t)(cell >> 32), (uint32_t)draw, (uint32_t)(draw >> 32), g.key0, g.key1, r);
    uint64_t rest = cell;
    float v[3], w[3];
#pragma unroll
    for (int k = 2; k >= 0; --k) {
        if (k >= g.dim) continue;
        const float* __restrict__ ed = k == 0 ? e0 : (k == 1 ? e1 : e2);
        const uint64_t s = (uint64_t)g.shape[k];
        const uint64_t q = rest / s;
        const uint32_t ik = (uint32_t)(rest - q * s);         // < shape[k]: edges_k holds shape[k] + 1 entries
        rest = q;
        const float a = ed[ik], b = ed[ik + 1];
        const float u = (float)(r[k] >> 8) * 0x1p-24f;
        w[k] = b - a;
        float xv = smp_mul_then_add(a, u, w[k]);
        xv = xv < g.clip_lo[k] ? g.clip_lo[k] : xv;
        xv = xv > g.clip_hi[k] ? g.clip_hi[k] : xv;
        v[k] = xv;
    }
    float qv = w[0];
#pragma unroll
    for (int k = 1; k < 3; ++k) {
        if (k >= g.dim) continue;
        qv = qv * w[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= g.dim) continue;
        x[j * g.dim + k] = v[k];
    }
    if (qw) qw[j] = qv;
}

// ---- residual-adaptive allocation (gpe_sampler_adaptive) -------------------------------------------------------------------------------
// The cells of a graded grid become BLOCKS that hold a varying number of rows: block b (row-major, last axis fastest) holds rows
// [off[b], off[b + 1]) of a buffer of fixed length N, every one of them a uniformly placed point of the block with weight v_b / n_b.
// Behind every `every` steps the engine evaluates the PDE residual on the set it holds (the forward-only path of gpe_residual) and
//   k_block_mass             m_b = sum over the block's rows of q_i * sum_c r_{i,c}^2, fp64, fixed order
//   k_adaptive_alloc         M = sum m_b (fixed order); counts n_b and offsets from the masses and the block volumes, in integers
//   k_sampler_draw_adaptive  the rows and their weights from the offsets
// run back to back on the engine's stream.  gpe_pinn/sampler.py (adaptive_counts, adaptive_points, adaptive_weights) restates the
// last two in numpy / Python integers, bit for bit; include/gpe_hip.h states the arithmetic.  No atomics; plain vector stores only.
// Bound on the block count: B <= SMP_AD_MAX_POINTS = 2^22.  The bind refuses N > 2^22 and B * n_min > N with n_min >= 1, so no larger B
// passes; k_adaptive_alloc is one workgroup whose threads each scan cdiv(B, SMP_AD_THREADS) consecutive blocks (at most 4096).
#define SMP_AD_MAX_POINTS (1 << 22)
#define SMP_AD_THREADS 1024
#define SMP_MASS_THREADS 256                       // k_block_mass: four waves, one small block each or one large block together
#define SMP_MASS_BIG 1024                          // ... rows from which a block is "large"
#define SMP_OFF_LDS 4096                           // k_sampler_draw_adaptive stages up to this many offsets in LDS

struct AdaptiveDev {                               // engine-owned, allocated at the bind
    double* mass;                                  // [B + 1]: m_b, then M
    int32_t* count;                                // [B]
    int32_t* off;                                  // [B + 1]: exclusive prefix sum of count; off[B] = N
    const float* vol;                              // [B]: v_b, the graded sampler's fp32 cell volume
    uint64_t* share;                               // [B]: k_b, kept by k_adaptive_alloc between its two passes
    int32_t B, N, n_min, s;                        // s = uniform_per_1024
    double V;                                      // sampler.graded_total(edges)
};

GPE_DEV double smp_wave_sum(double v) {            // wave64 butterfly: every lane ends with the same total, formed in one fixed tree
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

GPE_DEV double smp_row_mass(const float* __restrict__ resid, const float* __restrict__ qw, int n_out, int64_t i) {
    double s = 0.0;
    for (int c = 0; c < n_out; ++c) { const double r = (double)resid[i * n_out + c]; s += r * r; }
    return (double)qw[i] * s;
}

// mass[b] <- sum_{i in block b} q_i * sum_c r_{i,c}^2.  A workgroup takes four consecutive blocks (then the next four a grid further on).
// Every wave reads the four row ranges from `off`, so the choice below is made on the device and is the same in all four waves:
//   fewer than SMP_MASS_BIG rows   wave w reduces block 4g + w alone: lane l adds rows l, l + 64, ... in that order, then the butterfly
//   more                           the whole workgroup reduces it: thread t adds rows t, t + 256, ..., the butterfly per wave, and the
//                                  four wave totals are added in wave order
// The term of a row is double(r)^2 (exact: 48 bits), added over the outputs in fp64, times double(q): exactly what a host sum over
// the fp32 residuals forms in fp64, so only the order of the additions over the rows differs from any other fixed-order sum.
__global__ __launch_bounds__(SMP_MASS_THREADS) void k_block_mass(const float* __restrict__ resid, const float* __restrict__ qw,
                                                                 const int32_t* __restrict__ off, int n_out, int B,
                                                                 double* __restrict__ mass) {
    __shared__ double part[SMP_MASS_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t g0 = (int64_t)blockIdx.x * 4; g0 < B; g0 += (int64_t)gridDim.x * 4) {
        const int64_t b = g0 + wave;
        if (b < B) {
            const int lo = off[b], hi = off[b + 1];
            if (hi - lo < SMP_MASS_BIG) {
                double s = 0.0;
                for (int i = lo + lane; i < hi; i += 64) s += smp_row_mass(resid, qw, n_out, i);
                s = smp_wave_sum(s);
                if (lane == 0) mass[b] = s;
            }
        }
        for (int k = 0; k < 4; ++k) {              // (g0 + k, lo and hi are uniform over the workgroup: so are the barriers)
            const int64_t bk = g0 + k;
            if (bk >= B) break;
            const int lo = off[bk], hi = off[bk + 1];
            if (hi - lo < SMP_MASS_BIG) continue;
            double s = 0.0;
            for (int i = lo + (int)threadIdx.x; i < hi; i += SMP_MASS_THREADS) s += smp_row_mass(resid, qw, n_out, i);
            s = smp_wave_sum(s);
            if (lane == 0) part[wave] = s;
            __syncthreads();
            if (threadIdx.x == 0) {
                double t = part[0];
                for (int w = 1; w < SMP_MASS_THREADS / 64; ++w) t += part[w];
                mass[bk] = t;
            }
            __syncthreads();
        }
    }
}

// k_b of one block: (1024 - s) * floor(m_b / M * 2^30) + s * floor(v_b / V * 2^30) -- two IEEE fp64 divisions, two exact scalings by a
// power of two, two truncations of values in [0, 2^30]; everything behind them is unsigned 64-bit integer arithmetic
GPE_DEV uint64_t smp_share(const AdaptiveDev& a, int b, bool ok, double M) {
    const uint64_t kA = ok ? (uint64_t)floor(a.mass[b] / M * 0x1p30) : 0ull;
    const uint64_t kV = (uint64_t)floor((double)a.vol[b] / a.V * 0x1p30);
    return (uint64_t)(1024 - a.s) * kA + (uint64_t)a.s * kV;
}

// One workgroup.  M: thread t adds m_t, m_{t + 1024}, ... in that order, the butterfly per wave, the 16 wave totals in wave order; a NaN
// or inf anywhere ends in M (the masses are sums of non-negative terms), and M == 0, NaN or inf selects the allocation by volume.
// Scan: thread t owns the consecutive blocks [t * chunk, (t + 1) * chunk); the totals of the chunks are scanned in LDS (Hillis-Steele,
// 10 rounds) -- integer sums, so K_b is the same number whichever way it is bracketed -- and every thread walks its chunk again with
// K_b running:  n_b = n_min + (K_{b+1} R) / K_B - (K_b R) / K_B,  off_b = b n_min + (K_b R) / K_B  (K_B <= 2^40, R < 2^22).
// The first walk leaves k_b in a.share, so the two fp64 divisions of a block are made once.
// Cost: one workgroup, and with chunk > 1 neighbouring lanes are `chunk` blocks apart (uncoalesced).  Up to B = 1 024 every thread owns one
// block and the accesses are coalesced: a few microseconds.  At the bound B = 2^22 a thread walks 4 096 blocks twice -- two divisions
// and two 64-bit integer divisions per block, about 50 MB of strided traffic through one CU: of the order of 10 ms, once per `every`
// steps.  A grid of blocks that fine is outside what the sampler is for (a block wants tens of rows); a multi-workgroup scan is the
// remedy should one be needed.
__global__ __launch_bounds__(SMP_AD_THREADS) void k_adaptive_alloc(AdaptiveDev a) {
    __shared__ double wsum[SMP_AD_THREADS / 64];
    __shared__ double Msh;
    __shared__ uint64_t scan[2][SMP_AD_THREADS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double s = 0.0;
    for (int b = t; b < a.B; b += SMP_AD_THREADS) s += a.mass[b];
    s = smp_wave_sum(s);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (t == 0) {
        double m = wsum[0];
        for (int w = 1; w < SMP_AD_THREADS / 64; ++w) m += wsum[w];
        Msh = m;
    }
    __syncthreads();
    const double M = Msh;
    const bool ok = (M > 0.0) && (M < (double)INFINITY);
    const int chunk = (a.B + SMP_AD_THREADS - 1) / SMP_AD_THREADS;
    const int b0 = min(t * chunk, a.B), b1 = min(b0 + chunk, a.B);
    uint64_t mine = 0;
    for (int b = b0; b < b1; ++b) { const uint64_t k = smp_share(a, b, ok, M); a.share[b] = k; mine += k; }
    int cur = 0;
    scan[0][t] = mine;
    __syncthreads();
    for (int d = 1; d < SMP_AD_THREADS; d <<= 1) {
        scan[cur ^ 1][t] = scan[cur][t] + (t >= d ? scan[cur][t - d] : 0ull);
        cur ^= 1;
        __syncthreads();
    }
    const uint64_t KB = scan[cur][SMP_AD_THREADS - 1];       // > 0: the bind checked the volume shares
    uint64_t K = scan[cur][t] - mine;                        // exclusive
    const uint64_t R = (uint64_t)(a.N - (int64_t)a.B * a.n_min);
    for (int b = b0; b < b1; ++b) {
        const uint64_t k = a.share[b];               // (written by this thread above)
        const uint64_t q0 = KB ? (K * R) / KB : 0ull, q1 = KB ? ((K + k) * R) / KB : 0ull;
        a.count[b] = (int32_t)((uint64_t)a.n_min + q1 - q0);
        a.off[b] = (int32_t)((uint64_t)b * (uint64_t)a.n_min + q0);
        K += k;
    }
    if (t == 0) { a.off[a.B] = a.N; a.mass[a.B] = M; }
}

// x [N][dim], qw [N] <- draw `draw`.  Row j: block b = upper_bound(off, j) - 1 (offsets staged in LDS when B + 1 <= SMP_OFF_LDS), local
// index l = j - off[b]; Philox counter (b, l, draw lo, draw hi), key (seed lo, seed hi), output word k for axis k; per axis u, w, x and
// the clip exactly as k_sampler_draw_graded; q = float(double(v_b) / double(n_b)): one IEEE fp64 division, one conversion.
__global__ __launch_bounds__(SMP_THREADS) void k_sampler_draw_adaptive(SamplerGrid g, const float* __restrict__ e0, const float* __restrict__ e1,
                                                                       const float* __restrict__ e2, AdaptiveDev a, uint64_t draw,
                                                                       float* __restrict__ x, float* __restrict__ qw) {
    __shared__ int32_t soff[SMP_OFF_LDS];
    const bool staged = a.B + 1 <= SMP_OFF_LDS;              // (uniform over the grid)
    if (staged) {
        for (int i = threadIdx.x; i <= a.B; i += SMP_THREADS) soff[i] = a.off[i];
        __syncthreads();
    }
    const int64_t j = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (j >= a.N) return;
    const int32_t* __restrict__ off = staged ? soff : a.off;
    int lo = 0, hi = a.B;                                    // off[lo] <= j < off[hi] throughout (off[0] = 0, off[B] = N)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= j) lo = mid; else hi = mid;
    }
    const uint32_t b = (uint32_t)lo, l = (uint32_t)(j - off[lo]);
    uint32_t r[4];
    philox4x32_10(b, l, (uint32_t)draw, (uint32_t)(draw >> 32), g.key0, g.key1, r);
    uint32_t rest = b;
    float v[3];
#pragma unroll
    for (int k = 2; k >= 0; --k) {
        if (k >= g.dim) continue;
        const float* __restrict__ ed = k == 0 ? e0 : (k == 1 ? e1 : e2);
        const uint32_t s = (uint32_t)g.shape[k];
        const uint32_t q = rest / s;
        const uint32_t ik = rest - q * s;                    // < shape[k]: edges_k holds shape[k] + 1 entries
        rest = q;
        const float ea = ed[ik], eb = ed[ik + 1];
        const float u = (float)(r[k] >> 8) * 0x1p-24f;
        const float w = eb - ea;
        float xv = smp_mul_then_add(ea, u, w);
        xv = xv < g.clip_lo[k] ? g.clip_lo[k] : xv;
        xv = xv > g.clip_hi[k] ? g.clip_hi[k] : xv;
        v[k] = xv;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= g.dim) continue;
        x[j * g.dim + k] = v[k];
    }
    qw[j] = (float)((double)a.vol[b] / (double)a.count[b]);
}
