// gpe_potential.h -- analytic potential terms: the table a caller binds with gpe_potential_terms, its host check, the evaluator and the
// kernel that fills an engine-owned V array from it.  The step never sees the table: it runs on the GPE_POT_PRECOMPUTED path every kernel
// family already has (Vpre[m]), on an array this kernel wrote -- at every bind and directly behind every redraw of a sampler.  Phys and
// potential_at (gpe_common.h) are untouched, so no forward, head, seed or reverse kernel compiles differently.
//
// A term is (kind, a, w[3], c[3]).  With t_k = w_k (x_k - c_k) for k < dim and s = sum_k t_k^2 accumulated as s = fmaf(t_k, t_k, s) in
// ascending k -- the arithmetic of potential_at's harmonic case, so ONE QUAD term gives GPE_POT_HARMONIC's bits --
//   QUAD     a s                        QUARTIC  a s s                     GAUSS   a expf(-s)
//   LATTICE  a sum_{k: w_k != 0} cosf(t_k)^2                              LINEAR  a sum_k t_k
// and V(x) = sum_j term_j(x) in fp32, added in table order starting from 0.f.
//
// potential_terms_check and potential_terms_at (host instance) need nothing of HIP: tests/potential_selftest.cpp compiles this header
// alone with g++, under the host sanitizers.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include "../../include/gpe_hip.h"

#if defined(__HIPCC__)
#define GPE_HD __host__ __device__ inline
#else
#define GPE_HD inline
#endif

static_assert(sizeof(gpe_pot_term) == 32, "gpe_pot_term: 32 bytes (include/gpe_hip.h, gpe_pinn/_capi.py)");

struct PotTable { gpe_pot_term t[GPE_MAX_POT_TERMS]; };      // 512 bytes: the by-value argument of k_potential_terms, and of that kernel only

// V at one point; xv holds dim coordinates.  n <= GPE_MAX_POT_TERMS and dim <= 3 are the caller's to have established.
GPE_HD float potential_terms_at(const gpe_pot_term* table, int n, int dim, const float* xv) {
    float V = 0.f;
    for (int j = 0; j < n; ++j) {
        const gpe_pot_term& q = table[j];
        float t[3] = {0.f, 0.f, 0.f};
        float s = 0.f;
        for (int k = 0; k < dim; ++k) { t[k] = q.w[k] * (xv[k] - q.c[k]); s = fmaf(t[k], t[k], s); }
        float v = 0.f;
        switch (q.kind) {
            case GPE_TERM_QUAD: v = q.a * s; break;
            case GPE_TERM_QUARTIC: v = q.a * s * s; break;
            case GPE_TERM_GAUSS: v = q.a * expf(-s); break;
            case GPE_TERM_LATTICE: {
                float l = 0.f;
                for (int k = 0; k < dim; ++k) if (q.w[k] != 0.f) { const float c = cosf(t[k]); l += c * c; }
                v = q.a * l;
                break;
            }
            case GPE_TERM_LINEAR: {
                float l = 0.f;
                for (int k = 0; k < dim; ++k) l += t[k];
                v = q.a * l;
                break;
            }
            default: break;                      // (potential_terms_check lets no other kind in)
        }
        V += v;
    }
    return V;
}

#if defined(__HIPCC__)
#define POT_THREADS 256
// V[i] of row i of x [n_rows][dim]: one thread per row, 64-bit row index
__global__ __launch_bounds__(POT_THREADS) void k_potential_terms(PotTable table, int n_terms, int dim, const float* __restrict__ x, int64_t n_rows,
                                                                 float* __restrict__ V) {
    const int64_t i = (int64_t)blockIdx.x * POT_THREADS + threadIdx.x;
    if (i >= n_rows) return;
    float xv[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < dim; ++k) xv[k] = x[i * dim + k];
    V[i] = potential_terms_at(table.t, n_terms, dim, xv);
}
#endif

static inline int pot_refuse(std::string* msg, int code, const char* fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    *msg = b;
    return code;
}

// What gpe_potential_terms refuses of a table, in a fixed order (a table wrong in several ways reports the first); reads terms[0 .. n)
// only once n is known to lie in 1 .. GPE_MAX_POT_TERMS.  dim: the network's input dimension.
static inline int potential_terms_check(const gpe_pot_term* terms, int n, int dim, std::string* msg) {
    if (!terms) return pot_refuse(msg, GPE_ERR_INVALID, "potential_terms: no table");
    if (n < 1 || n > GPE_MAX_POT_TERMS) return pot_refuse(msg, GPE_ERR_INVALID, "potential_terms: n_terms = %d, need 1 .. %d", n, GPE_MAX_POT_TERMS);
    for (int j = 0; j < n; ++j) {
        const gpe_pot_term& q = terms[j];
        if (q.kind < GPE_TERM_QUAD || q.kind > GPE_TERM_LINEAR) return pot_refuse(msg, GPE_ERR_INVALID, "potential_terms: term %d has unknown kind %d", j, (int)q.kind);
        if (!std::isfinite(q.a)) return pot_refuse(msg, GPE_ERR_INVALID, "potential_terms: term %d: a is not finite", j);
        bool any_w = false;
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(q.w[k])) return pot_refuse(msg, GPE_ERR_INVALID, "potential_terms: term %d: w[%d] is not finite", j, k);
            if (!std::isfinite(q.c[k])) return pot_refuse(msg, GPE_ERR_INVALID, "potential_terms: term %d: c[%d] is not finite", j, k);
            if (k >= dim && (q.w[k] != 0.f || q.c[k] != 0.f))
                return pot_refuse(msg, GPE_ERR_INVALID, "potential_terms: term %d: w[%d] / c[%d] must be 0 on an axis the network does not have (dim = %d)", j, k, k, dim);
            any_w = any_w || q.w[k] != 0.f;
        }
        if (q.kind == GPE_TERM_LATTICE && !any_w) return pot_refuse(msg, GPE_ERR_INVALID, "potential_terms: term %d: a lattice with every w[k] == 0 has no axis", j);
    }
    return GPE_OK;
}
