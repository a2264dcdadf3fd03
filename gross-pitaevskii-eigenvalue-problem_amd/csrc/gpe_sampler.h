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
