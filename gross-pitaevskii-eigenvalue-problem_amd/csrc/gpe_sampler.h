// gpe_sampler.h -- stratified collocation sets drawn on the device (include/gpe_hip.h: gpe_bind_sampler and its kin).  One uniformly
// placed point per cell of a tensor-product grid, from a counter-based generator, written in place into the engine's own point buffer.
// Replaces the host loop of tools/accuracy_nd.py:run_epochs (16 jittered numpy copies of the grid, uploaded, cycled with
// gpe_bind_points); the reference has no counterpart: it trains on one fixed grid.
//
// Every kernel here is one thread per row, one Philox call per thread, plain vector stores (global_store_dword) only.  They differ in
// which cell a row is and in how an axis places its point; the arithmetic of a row is stated once, at the pieces below, and
// gpe_pinn/sampler.py restates it in numpy, bit for bit:
//   kernel                        row j is cell                 axis step    sampler.py
//   k_sampler_draw                first_cell + j                uniform      stratified_points
//   k_sampler_draw_graded         first_cell + j                graded       graded_points / graded_weights
//   k_sampler_draw_cells          cells[first + j]              uniform      cells_points  (= stratified_points(...)[cells])
//   k_sampler_draw_graded_cells   cells[first + j]              graded       cells_points / cells_weights
//   k_sampler_draw_adaptive       block b, local index l        graded       adaptive_points / adaptive_weights  (further down)
// Cells are numbered row-major, last axis fastest, so contiguous blocks of cells (or of a list) held by different ranks are, together,
// the set one rank would hold.
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

// ---- the pieces of a row ------------------------------------------------------------------------------------------------------------
// words: Philox4x32-10, counter (c lo, c hi, draw lo, draw hi), key (seed lo, seed hi); output word k serves axis k.  The grid kernels
// count by the cell (64 bits); the adaptive kernel by (block, local index), one word each.
GPE_DEV void smp_words(const SamplerGrid& g, uint32_t c0, uint32_t c1, uint64_t draw, uint32_t (&r)[4]) {
    philox4x32_10(c0, c1, (uint32_t)draw, (uint32_t)(draw >> 32), g.key0, g.key1, r);
}

// row-major split, last axis fastest: takes axis k's index off what is left of the cell.  64-bit divisions (a rank's cells fit int64, a
// grid may hold more than 2^32); the index is < shape[k] <= 2^24
GPE_DEV uint32_t smp_split(uint64_t& rest, int64_t shape_k) {
    const uint64_t s = (uint64_t)shape_k;
    const uint64_t q = rest / s;
    const uint32_t ik = (uint32_t)(rest - q * s);
    rest = q;
    return ik;
}

// u = float(word >> 8) * 2^-24: exact, 24 bits, in [0, 1)
GPE_DEV float smp_unit(uint32_t word) { return (float)(word >> 8) * 0x1p-24f; }

// by comparisons, not fmin / fmax: no choice between +0 and -0
GPE_DEV float smp_clip(const SamplerGrid& g, int k, float xv) {
    xv = xv < g.clip_lo[k] ? g.clip_lo[k] : xv;
    xv = xv > g.clip_hi[k] ? g.clip_hi[k] : xv;
    return xv;
}

// uniform axis: t = float(i_k) + u, one rounded fp32 add (i_k < 2^24, checked at the bind); x = lo[k] + t * h[k], one rounded multiply,
// one rounded add, never an fma; the clip
GPE_DEV float smp_axis_uniform(const SamplerGrid& g, int k, uint32_t ik, uint32_t word) {
    const float u = smp_unit(word);
    const float t = (float)ik + u;
    return smp_clip(g, k, smp_mul_then_add(g.lo[k], t, g.h[k]));
}

// graded axis: cell i_k spans [a, b] = [ed[i_k], ed[i_k + 1]] of the caller's edges (shape[k] + 1 entries, so the reads stay inside);
// w = b - a, one rounded fp32 subtraction: the cell's width; x = a + u * w, one rounded multiply, one rounded add, never an fma; the
// clip.  g.lo / g.h are not read.
GPE_DEV float smp_axis_graded(const SamplerGrid& g, int k, const float* __restrict__ ed, uint32_t ik, uint32_t word, float& w) {
    const float a = ed[ik], b = ed[ik + 1];
    const float u = smp_unit(word);
    w = b - a;
    return smp_clip(g, k, smp_mul_then_add(a, u, w));
}

// the cell's volume, a graded row's quadrature weight: w_0, then * w_1, then * w_2 -- rounded fp32 multiplies in axis order
GPE_DEV float smp_volume(const SamplerGrid& g, const float (&w)[3]) {
    float qv = w[0];
#pragma unroll
    for (int k = 1; k < 3; ++k) {
        if (k >= g.dim) continue;
        qv = qv * w[k];
    }
    return qv;
}

// x [n][dim] row j <- v
GPE_DEV void smp_store(const SamplerGrid& g, const float (&v)[3], int64_t j, float* __restrict__ x) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= g.dim) continue;
        x[j * g.dim + k] = v[k];
    }
}

// ... and, for the two uniform forms, xs (NULL: none) [2n][dim] rows j and n + j <- v and -v: the symmetry batch [x ; -x]
GPE_DEV void smp_store_sym(const SamplerGrid& g, const float (&v)[3], int64_t j, int64_t n, float* __restrict__ x, float* __restrict__ xs) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= g.dim) continue;
        x[j * g.dim + k] = v[k];
        if (xs) { xs[j * g.dim + k] = v[k]; xs[(n + j) * g.dim + k] = -v[k]; }
    }
}

// ---- the two rows of the grid kernels ---------------------------------------------------------------------------------------------------
// row j of x (and of [x ; -x]) <- draw `draw` of cell `cell` of the uniform grid
GPE_DEV void smp_row_uniform(const SamplerGrid& g, uint64_t cell, int64_t j, int64_t n, uint64_t draw, float* __restrict__ x,
                             float* __restrict__ xs) {
    uint32_t r[4];
    smp_words(g, (uint32_t)cell, (uint32_t)(cell >> 32), draw, r);
    uint64_t rest = cell;
    float v[3];
#pragma unroll
    for (int k = 2; k >= 0; --k) {
        if (k >= g.dim) continue;
        v[k] = smp_axis_uniform(g, k, smp_split(rest, g.shape[k]), r[k]);
    }
    smp_store_sym(g, v, j, n, x, xs);
}

// ... of the graded grid; qw (NULL: not wanted) [n] row j <- the cell's volume.  The weights do not depend on the draw: the bind writes
// them, the redraws pass NULL.
GPE_DEV void smp_row_graded(const SamplerGrid& g, const float* __restrict__ e0, const float* __restrict__ e1, const float* __restrict__ e2,
                            uint64_t cell, int64_t j, uint64_t draw, float* __restrict__ x, float* __restrict__ qw) {
    uint32_t r[4];
    smp_words(g, (uint32_t)cell, (uint32_t)(cell >> 32), draw, r);
    uint64_t rest = cell;
    float v[3], w[3];
#pragma unroll
    for (int k = 2; k >= 0; --k) {
        if (k >= g.dim) continue;
        v[k] = smp_axis_graded(g, k, k == 0 ? e0 : (k == 1 ? e1 : e2), smp_split(rest, g.shape[k]), r[k], w[k]);
    }
    smp_store(g, v, j, x);
    if (qw) qw[j] = smp_volume(g, w);
}

// ---- the grid kernels: which cell is row j ------------------------------------------------------------------------------------------
// cells [first_cell, first_cell + n) of the grid ...
__global__ __launch_bounds__(SMP_THREADS) void k_sampler_draw(SamplerGrid g, int64_t first_cell, int64_t n, uint64_t draw,
                                                              float* __restrict__ x, float* __restrict__ xs) {
    const int64_t j = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (j >= n) return;
    smp_row_uniform(g, (uint64_t)(first_cell + j), j, n, draw, x, xs);
}

__global__ __launch_bounds__(SMP_THREADS) void k_sampler_draw_graded(SamplerGrid g, const float* __restrict__ e0, const float* __restrict__ e1,
                                                                     const float* __restrict__ e2, int64_t first_cell, int64_t n, uint64_t draw,
                                                                     float* __restrict__ x, float* __restrict__ qw) {
    const int64_t j = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (j >= n) return;
    smp_row_graded(g, e0, e1, e2, (uint64_t)(first_cell + j), j, draw, x, qw);
}

// ... or rows [first, first + n) of `cells` (gpe_sampler_cells), the engine-owned copy of the caller's strictly ascending list (a disk,
// a ball, any mask: gpe_pinn/sampler.py ball_cells / mask_cells).  The bind checked every entry against [0, prod shape), so the per-axis
// index stays below shape[k] and the edge reads stay inside their arrays.  The 8-byte index loads of a wave are consecutive (one
// coalesced global_load_dwordx2 each).
__global__ __launch_bounds__(SMP_THREADS) void k_sampler_draw_cells(SamplerGrid g, const int64_t* __restrict__ cells, int64_t first, int64_t n,
                                                                    uint64_t draw, float* __restrict__ x, float* __restrict__ xs) {
    const int64_t j = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (j >= n) return;
    smp_row_uniform(g, (uint64_t)cells[first + j], j, n, draw, x, xs);
}

__global__ __launch_bounds__(SMP_THREADS) void k_sampler_draw_graded_cells(SamplerGrid g, const float* __restrict__ e0, const float* __restrict__ e1,
                                                                           const float* __restrict__ e2, const int64_t* __restrict__ cells,
                                                                           int64_t first, int64_t n, uint64_t draw, float* __restrict__ x,
                                                                           float* __restrict__ qw) {
    const int64_t j = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (j >= n) return;
    smp_row_graded(g, e0, e1, e2, (uint64_t)cells[first + j], j, draw, x, qw);
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
// index l = j - off[b]; the words are counted by (b, l) and b splits in 32 bits (B <= 2^22); per axis smp_axis_graded, the step of the
// graded grid kernels; q = float(double(v_b) / double(n_b)): one IEEE fp64 division, one conversion.
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
    smp_words(g, b, l, draw, r);
    uint32_t rest = b;
    float v[3];
#pragma unroll
    for (int k = 2; k >= 0; --k) {
        if (k >= g.dim) continue;
        const uint32_t s = (uint32_t)g.shape[k];
        const uint32_t q = rest / s;
        const uint32_t ik = rest - q * s;                    // < shape[k]
        rest = q;
        float w;
        v[k] = smp_axis_graded(g, k, k == 0 ? e0 : (k == 1 ? e1 : e2), ik, r[k], w);
    }
    smp_store(g, v, j, x);
    qw[j] = (float)((double)a.vol[b] / (double)a.count[b]);
}
