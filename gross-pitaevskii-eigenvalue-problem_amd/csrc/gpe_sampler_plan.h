// gpe_sampler_plan.h -- the host-only part of a sampler bind (gpe_bind_sampler, gpe_bind_sampler_graded, gpe_sampler_adaptive,
// gpe_sampler_cells): everything that reads nothing but the caller's host data.  No HIP here, so tests/sampler_plan_selftest.cpp
// compiles it alone, under the host sanitizers, and feeds it every refusal and a few accepted grids.
//
// sampler_plan either refuses (a gpe_status and its text; nothing else is written) or fills a SamplerPlan: the row count, the length of
// the edge array, W (the volume of the whole grid, or of the whole list) and the adaptive sampler's block volumes.  The checks come in
// a fixed order -- a call that is wrong in several ways reports the first -- and the two places that index the caller's edges by a
// cell (cell_volume) are reached only behind BOTH scans: the list scan bounds every cell by prod shape, so its per-axis index stays
// below shape[k], and the edge scan found shape[k] + 1 readable entries per used axis.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/gpe_hip.h"

struct AdaptiveArgs { int64_t n_points; int32_t n_min, s; };          // gpe_sampler_adaptive: rows of the buffer, floor per block, uniform_per_1024
struct CellsArgs { const int64_t* h_cells; int64_t n_cells; };        // gpe_sampler_cells: the caller's list

struct SamplerPlan {
    int64_t n_rows = 0;                          // rows of the point buffer: n_local, or the adaptive sampler's n_points
    int64_t n_edges = 0;                         // sum over the used axes of shape[k] + 1; 0 without edges
    double w_grid = 1.0;                         // graded: W, the bound weights' total over all ranks (sampler.py graded_total / cells_total)
    std::vector<float> vol;                      // adaptive: the block volumes v_b (sampler.py graded_weights)
};

// the entry point's name in every message (edges NULL: the uniform grid; ad, cl: see above)
static inline const char* sampler_who(const float* const* edges, const AdaptiveArgs* ad, const CellsArgs* cl) {
    return cl ? "sampler_cells" : ad ? "sampler_adaptive" : edges ? "bind_sampler_graded" : "bind_sampler";
}

static inline int plan_refuse(std::string* msg, int code, const char* fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    *msg = b;
    return code;
}

// fp32 volume of cell c (row-major, last axis fastest) as the draw kernels form it: fp32 widths, rounded fp32 products in axis order.
// Checks nothing: c < prod shape and shape[k] + 1 entries per used axis are the caller's to have established.
static inline float cell_volume(const float* const* edges, const int64_t* shape, int dim, int64_t cell) {
    int64_t rest = cell, ik[3] = {0, 0, 0};
    for (int k = dim - 1; k >= 0; --k) { ik[k] = rest % shape[k]; rest /= shape[k]; }
    float v = edges[0][ik[0] + 1] - edges[0][ik[0]];
    for (int k = 1; k < dim; ++k) { const float w = edges[k][ik[k] + 1] - edges[k][ik[k]]; v = v * w; }
    return v;
}

// spec: every, shape against the network's `dim` input axes, lo / hi / clip; `cells` <- the grid's cell count.  w_sym (the engine
// keeps a symmetry batch) is the one fact of the engine judged here and not before: its refusal has always come second.
static inline int plan_check_spec(const char* who, int dim, bool w_sym, const gpe_sampler_spec* sp, bool graded, double* cells, std::string* msg) {
    if (sp->every <= 0) return plan_refuse(msg, GPE_ERR_INVALID, "%s: every = %lld, need > 0", who, (long long)sp->every);
    if (graded && w_sym) return plan_refuse(msg, GPE_ERR_INVALID, "%s: the symmetry batch has no quadrature weights (w_sym != 0)", who);
    *cells = 1.0;
    for (int k = 0; k < 3; ++k) {
        if ((sp->shape[k] > 0) != (k < dim))
            return plan_refuse(msg, GPE_ERR_INVALID, "%s: shape must use exactly the network's %d input axes (shape[%d] = %lld)", who, dim, k, (long long)sp->shape[k]);
        if (k >= dim) continue;
        if (sp->shape[k] > (1 << 24)) return plan_refuse(msg, GPE_ERR_INVALID, "%s: shape[%d] = %lld, at most 2^24 cells per axis", who, k, (long long)sp->shape[k]);
        if (!(sp->hi[k] > sp->lo[k])) return plan_refuse(msg, GPE_ERR_INVALID, "%s: hi <= lo on axis %d", who, k);
        if (!(sp->clip_hi[k] >= sp->clip_lo[k])) return plan_refuse(msg, GPE_ERR_INVALID, "%s: clip_hi < clip_lo on axis %d", who, k);
        *cells *= (double)sp->shape[k];
    }
    return GPE_OK;
}

// the list: strictly ascending cells of this grid; the rows: a block of the list
static inline int plan_scan_list(const char* who, int dim, const gpe_sampler_spec* sp, const CellsArgs* cl, double cells, std::string* msg) {
    unsigned __int128 total = 1;                 // (up to 2^72 cells: beyond int64, and a double would round the last cell onto the bound)
    for (int k = 0; k < dim; ++k) total *= (unsigned __int128)sp->shape[k];
    for (int64_t i = 0; i < cl->n_cells; ++i) {
        const int64_t c = cl->h_cells[i];
        if (c < 0 || (unsigned __int128)c >= total)
            return plan_refuse(msg, GPE_ERR_INVALID, "%s: cells[%lld] = %lld outside the grid's %.0f cells", who, (long long)i, (long long)c, cells);
        if (i > 0 && !(c > cl->h_cells[i - 1]))
            return plan_refuse(msg, GPE_ERR_INVALID, "%s: the list is not strictly ascending at position %lld (%lld after %lld)", who, (long long)i,
                               (long long)c, (long long)cl->h_cells[i - 1]);
    }
    if (sp->first_cell < 0 || sp->n_local <= 0 || sp->n_local > cl->n_cells || sp->first_cell > cl->n_cells - sp->n_local)
        return plan_refuse(msg, GPE_ERR_INVALID, "%s: rows [%lld, %lld + %lld) outside the list's %lld", who, (long long)sp->first_cell,
                           (long long)sp->first_cell, (long long)sp->n_local, (long long)cl->n_cells);
    return GPE_OK;
}

// strictly increasing finite edges that start at lo and end at hi; w_grid <- the product over the axes of the fp64 sums, in index order,
// of the fp32 widths -- of the WHOLE grid, whichever block of cells this rank holds
static inline int plan_scan_edges(const char* who, int dim, const gpe_sampler_spec* sp, const float* const* edges, SamplerPlan* p, std::string* msg) {
    double w_grid = 1.0;
    int64_t n_edges = 0;
    for (int k = 0; k < dim; ++k) {
        const float* ed = edges[k];
        if (!ed) return plan_refuse(msg, GPE_ERR_INVALID, "%s: no edges for axis %d", who, k);
        double wk = 0.0;
        for (int64_t i = 0; i <= sp->shape[k]; ++i) {
            if (!__builtin_isfinite(ed[i])) return plan_refuse(msg, GPE_ERR_INVALID, "%s: edge %lld of axis %d is not finite", who, (long long)i, k);
            if (i > 0 && !(ed[i] > ed[i - 1])) return plan_refuse(msg, GPE_ERR_INVALID, "%s: edges of axis %d do not increase at %lld", who, k, (long long)i);
            if (i > 0) { const float w = ed[i] - ed[i - 1]; wk += (double)w; }
        }
        if (ed[0] != sp->lo[k] || ed[sp->shape[k]] != sp->hi[k])
            return plan_refuse(msg, GPE_ERR_INVALID, "%s: lo / hi of axis %d are not its first / last edge", who, k);
        w_grid *= wk;
        n_edges += sp->shape[k] + 1;
    }
    p->w_grid = w_grid; p->n_edges = n_edges;
    return GPE_OK;
}

// dim: the network's input axes; w_sym: the engine keeps a symmetry batch; edges NULL: a uniform grid, else one host array per used axis;
// ad / cl NULL: not the adaptive / not the cell-subset sampler; max_points: SMP_AD_MAX_POINTS.  On a refusal *plan is left as it was.
static inline int sampler_plan(int dim, bool w_sym, const gpe_sampler_spec* sp, const float* const* edges, const AdaptiveArgs* ad,
                               const CellsArgs* cl, int64_t max_points, SamplerPlan* plan, std::string* msg) {
    const char* who = sampler_who(edges, ad, cl);
    SamplerPlan p;
    double cells = 1.0;
    int rc;
    if ((rc = plan_check_spec(who, dim, w_sym, sp, edges != nullptr, &cells, msg))) return rc;
    if (cl) {
        if ((rc = plan_scan_list(who, dim, sp, cl, cells, msg))) return rc;
    } else if (sp->first_cell < 0 || sp->n_local <= 0 || (double)sp->first_cell + (double)sp->n_local > cells)
        return plan_refuse(msg, GPE_ERR_INVALID, "%s: cells [%lld, %lld + %lld) outside the grid's %.0f", who, (long long)sp->first_cell,
                           (long long)sp->first_cell, (long long)sp->n_local, cells);
    p.n_rows = ad ? ad->n_points : sp->n_local;
    if (ad) {
        if (sp->first_cell != 0 || (double)sp->n_local != cells)
            return plan_refuse(msg, GPE_ERR_INVALID, "%s: single-rank, first_cell must be 0 and n_local the block count %.0f", who, cells);
        if (ad->n_points <= 0 || ad->n_points > max_points)
            return plan_refuse(msg, GPE_ERR_INVALID, "%s: n_points = %lld, need 1 .. 2^22", who, (long long)ad->n_points);
        if (ad->n_min < 1 || (double)sp->n_local * (double)ad->n_min > (double)ad->n_points)
            return plan_refuse(msg, GPE_ERR_INVALID, "%s: %lld blocks of at least n_min = %d rows do not fit %lld points", who, (long long)sp->n_local,
                               ad->n_min, (long long)ad->n_points);
        if (ad->s < 1 || ad->s > 1024) return plan_refuse(msg, GPE_ERR_INVALID, "%s: uniform_per_1024 = %d, need 1 .. 1024", who, ad->s);
    }
    if (edges && (rc = plan_scan_edges(who, dim, sp, edges, &p, msg))) return rc;
    // ---- both scans are behind us: from here a cell may index the edges ----
    if (edges && cl) {                           // W of the WHOLE list: the fp64 sum, in list order, of the fp32 cell volumes
        p.w_grid = 0.0;
        for (int64_t i = 0; i < cl->n_cells; ++i) p.w_grid += (double)cell_volume(edges, sp->shape, dim, cl->h_cells[i]);
    }
    if (edges && ad) {                           // the block volumes; their shares must not all truncate to zero (K_B > 0 in k_adaptive_alloc)
        p.vol.resize((size_t)sp->n_local);
        uint64_t kv_sum = 0;
        for (int64_t b = 0; b < sp->n_local; ++b) {
            const float v = cell_volume(edges, sp->shape, dim, b);
            p.vol[(size_t)b] = v;
            const double share = (double)v / p.w_grid * 0x1p30;
            if (share >= 0.0 && share <= 0x1p31) kv_sum += (uint64_t)share;
        }
        if (!(p.w_grid > 0.0) || !__builtin_isfinite(p.w_grid) || kv_sum == 0)
            return plan_refuse(msg, GPE_ERR_INVALID, "%s: the block volumes underflow or overflow fp32", who);
    }
    *plan = std::move(p);
    return GPE_OK;
}
