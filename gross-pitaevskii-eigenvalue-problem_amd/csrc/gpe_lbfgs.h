// gpe_lbfgs.h -- the kernels of the device-resident L-BFGS: torch.optim.LBFGS as the reference's pre-training tail and 2D hybrid driver
// take it, with or without the strong-Wolfe line search.  State and scalar rules (the freeze, the judged point, the line search's state
// machine) are gpe_lbfgs_rules.h; DESIGN.md ("L-BFGS") has the algebra.  An ITERATION (tests/lbfgs_ref.py) is three launches:
//   k_lbfgs_dots    y = g - g_prev and s = t d on the fly (rounded to fp32, as the rings hold them); their dot products with every live
//                   ring row and those of g, y.y, y.s, s.g, y.g, g.g, sum|g|, max|g|.  One wave per workgroup, grid a function of P
//                   alone, fixed element -> lane map, fp64 sums, one partial row per workgroup, no atomics: the same bits on every run.
//   k_lbfgs_coef    one workgroup: adds the rows in index order; torch's rules (push only if ys > 1e-10, pop the oldest at `history`,
//                   H_diag = ys / yy, first step min(1, 1/|g|_1) lr, no update if g.d > -tolerance_change); lbfgs_freeze on
//                   max|g| <= tolerance_grad, a non-finite loss or gradient, or loss < stop_loss (> 0); the Gram blocks S.Y and Y.Y in
//                   PHYSICAL slots (`head`: the next push; live: head - count .. head - 1 mod m), the two-loop recursion on COEFFICIENTS
//                   of d over {S_j, Y_j, g}, the tick's decisions (LbfgsTick) and the record.
//   k_lbfgs_apply   per element lbfgs_iterate, g_prev = g and the move.  A frozen iteration writes nothing, a skipped one all but theta.
// With the line search (tests/lbfgs_ls_ref.py) a TICK is a decision, then the iteration only if it ACCEPTS a point: always five launches,
// no decision read by the host.  k_ls_dots files g in a free slot, k_ls_decide calls ls_decide, the <true> instantiations take the ACCEPTED
// slot's gradient and loss or return at once (grid-uniform, LbfgsTick::action).
#pragma once
#include "gpe_lbfgs_rules.h"
#define LBFGS_E 8                               // elements per lane and tile
#define LBFGS_TILE (64 * LBFGS_E)
#define LBFGS_MAX_WG 128
#define LBFGS_PER_SLOT 5                        // S_j.g, Y_j.g, S_j.y, s.Y_j, y.Y_j
enum { LBD_YS = 0, LBD_YY, LBD_SG, LBD_YG, LBD_GG, LBD_G1, LBD_GMAX, LBD_BASE_COUNT = 8 };
enum { LSD_GTD = 0, LSD_G1, LSD_GMAX, LSD_DMAX, LSD_COUNT };

static inline int lbfgs_grid(int P) { const int g = (P + LBFGS_TILE - 1) / LBFGS_TILE; return g < LBFGS_MAX_WG ? g : LBFGS_MAX_WG; }
static inline int lbfgs_row(int m) { return LBFGS_PER_SLOT * m + LBD_BASE_COUNT; }

GPE_DEV bool lbfgs_live(int j, int head, int count, int m) {
    const int oldest = (head - count + m) % m;
    return ((j - oldest + m) % m) < count;
}
GPE_DEV double lbfgs_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
GPE_DEV const float* ls_slot_ptr(const LbfgsDev* st, const float* g_prev, int ld, int slot) {
    return slot == LS_START_SLOT ? g_prev : st->ls.slots + (size_t)slot * ld;
}
// theta0 + t d in fp64, rounded once; ONE expression for trial and accepted points, so that an accepted point is the trial's bits
GPE_DEV float ls_point(float theta0, double t, float d) { return (float)fma(t, (double)d, (double)theta0); }

template <bool LS>
__global__ __launch_bounds__(64) void k_lbfgs_dots(int P, int ld, int m, const float* __restrict__ grad, const float* __restrict__ g_prev,
                                                    const float* __restrict__ d, const float* __restrict__ S, const float* __restrict__ Y,
                                                    const LbfgsDev* __restrict__ st, double* __restrict__ part) {
    __shared__ double acc[LBFGS_PER_SLOT * LBFGS_MAX_HISTORY + LBD_BASE_COUNT];
    const int lane = threadIdx.x, W = LBFGS_PER_SLOT * m + LBD_BASE_COUNT;
    if constexpr (LS) {                                             // (grid-uniform) the accepted slot's gradient, or nothing to do
        if (st->tick.action != LS_ACT_ACCEPT) return;
        grad = ls_slot_ptr(st, g_prev, ld, st->tick.acc_slot);
    }
    const bool has_pair = st->n_iter >= 1;
    const int head = st->head, count = st->count;
    const double t = st->t;
    for (int v = lane; v < W; v += 64) acc[v] = 0.0;
    __syncthreads();
    for (int base = blockIdx.x * LBFGS_TILE; base < P; base += gridDim.x * LBFGS_TILE) {
        float g[LBFGS_E], s[LBFGS_E], y[LBFGS_E];
        double b[LBD_BASE_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < LBFGS_E; ++k) {
            const int i = base + k * 64 + lane;
            g[k] = 0.f; s[k] = 0.f; y[k] = 0.f;
            if (i < P) {
                g[k] = grad[i];
                if (has_pair) { y[k] = g[k] - g_prev[i]; s[k] = (float)(t * (double)d[i]); }
            }
            const double gd = g[k], sd = s[k], yd = y[k];
            b[LBD_YS] += yd * sd; b[LBD_YY] += yd * yd; b[LBD_SG] += sd * gd; b[LBD_YG] += yd * gd; b[LBD_GG] += gd * gd;
            b[LBD_G1] += fabs(gd); b[LBD_GMAX] = fmax(b[LBD_GMAX], fabs(gd));
        }
#pragma unroll
        for (int q = 0; q < LBD_GMAX; ++q) b[q] = lbfgs_wave_sum(b[q]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b[LBD_GMAX] = fmax(b[LBD_GMAX], __shfl_down(b[LBD_GMAX], o, 64));
        if (lane == 0) {
            double* a = acc + LBFGS_PER_SLOT * m;
            for (int q = 0; q < LBD_GMAX; ++q) a[q] += b[q];
            a[LBD_GMAX] = fmax(a[LBD_GMAX], b[LBD_GMAX]);
        }
        for (int j = 0; j < m; ++j) {
            if (!lbfgs_live(j, head, count, m)) continue;           // (uniform over the grid)
            const float* Sj = S + (size_t)j * ld;
            const float* Yj = Y + (size_t)j * ld;
            double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, c4 = 0.0;
#pragma unroll
            for (int k = 0; k < LBFGS_E; ++k) {
                const int i = base + k * 64 + lane;
                if (i < P) {
                    const double sj = Sj[i], yj = Yj[i];
                    c0 += sj * (double)g[k]; c1 += yj * (double)g[k]; c2 += sj * (double)y[k]; c3 += yj * (double)s[k]; c4 += yj * (double)y[k];
                }
            }
            c0 = lbfgs_wave_sum(c0); c1 = lbfgs_wave_sum(c1); c2 = lbfgs_wave_sum(c2); c3 = lbfgs_wave_sum(c3); c4 = lbfgs_wave_sum(c4);
            if (lane == 0) {
                double* a = acc + LBFGS_PER_SLOT * j;
                a[0] += c0; a[1] += c1; a[2] += c2; a[3] += c3; a[4] += c4;
            }
        }
    }
    __syncthreads();
    for (int v = lane; v < W; v += 64) part[(size_t)blockIdx.x * W + v] = acc[v];
}

// the record of an iteration (gpe_lbfgs_read), live or frozen: this evaluation, what was decided on it, and the state as it now stands
GPE_DEV void lbfgs_record(LbfgsDev* st, double loss, double gmax, double g1, double gtd, int skip, int push, double ys) {
    double* r = st->rec;
    r[LBR_LOSS] = loss; r[LBR_GMAX] = gmax; r[LBR_G1] = g1; r[LBR_T] = st->t; r[LBR_GTD] = gtd; r[LBR_N_ITER] = (double)st->n_iter;
    r[LBR_COUNT] = st->count; r[LBR_FROZEN] = st->frozen; r[LBR_SKIPPED] = skip; r[LBR_PUSHED] = push; r[LBR_YS] = ys;
    r[LBR_H_DIAG] = st->H_diag; r[LBR_HEAD] = st->head; r[LBR_PREV_LOSS] = st->prev_loss;
}

// SY[a * m + b] = S_a . Y_b, YY[a * m + b] = Y_a . Y_b over physical slots; coef = [cS (m) | cY (m) | c_g]
template <bool LS>
__global__ __launch_bounds__(256) void k_lbfgs_coef(int m, int n_part, LbfgsCfg cfg, LbfgsDev* __restrict__ st, const double* __restrict__ part,
                                                     double* __restrict__ SY, double* __restrict__ YY, double* __restrict__ ro,
                                                     double* __restrict__ coef, const gpe_scalars* __restrict__ last) {
    __shared__ double dots[LBFGS_PER_SLOT * LBFGS_MAX_HISTORY + LBD_BASE_COUNT];
    __shared__ double al[LBFGS_MAX_HISTORY], cs[LBFGS_MAX_HISTORY], w[LBFGS_MAX_HISTORY];
    __shared__ int s_mode, s_head, s_count, s_push, s_slot;
    __shared__ double s_H;
    const int tid = threadIdx.x, W = LBFGS_PER_SLOT * m + LBD_BASE_COUNT, B = LBFGS_PER_SLOT * m;
    if constexpr (LS) { if (st->tick.action != LS_ACT_ACCEPT) return; }
    for (int v = tid; v < W; v += 256) {
        double a = 0.0;
        if (v == B + LBD_GMAX) { for (int r = 0; r < n_part; ++r) a = fmax(a, part[(size_t)r * W + v]); }
        else { for (int r = 0; r < n_part; ++r) a += part[(size_t)r * W + v]; }
        dots[v] = a;
    }
    __syncthreads();
    const double loss = LS ? st->tick.f_acc : last->loss, g1 = dots[B + LBD_G1], gmax = dots[B + LBD_GMAX], gg = dots[B + LBD_GG];
    if (tid == 0) {
        int frozen = st->frozen;
        if (!frozen) {
            if (!(isfinite(loss) && isfinite(g1))) frozen = LBFGS_FROZEN_NONFINITE;
            else if (gmax <= cfg.tol_grad) frozen = LBFGS_FROZEN_GRAD;
            else if (cfg.stop_loss > 0.0 && loss < cfg.stop_loss) frozen = LBFGS_FROZEN_LOSS;      // (0: no such stop)
        }
        int head = st->head, count = st->count, push = 0, slot = 0, mode = 0;      // mode: 0 frozen, 1 first iteration, 2 later
        double H = st->H_diag;
        if (frozen) {                                               // (k_lbfgs_apply<true> leaves theta at the accepted point)
            lbfgs_freeze(st, frozen, LS);
            lbfgs_record(st, loss, gmax, g1, 0.0, 1, 0, 0.0);
        } else if (st->n_iter == 0) {
            mode = 1; head = 0; count = 0; H = 1.0;
        } else {
            mode = 2;
            const double ys = dots[B + LBD_YS];
            if (ys > 1e-10) {
                push = 1; slot = head;
                if (count < m) count += 1;                         // (at `history` the oldest pair sits in slot `head`: overwritten)
                head = (head + 1) % m;
                ro[slot] = 1.0 / ys;
                H = ys / dots[B + LBD_YY];
            }
        }
        s_mode = mode; s_head = head; s_count = count; s_push = push; s_slot = slot; s_H = H;
    }
    __syncthreads();
    const int mode = s_mode;
    if (mode == 0) return;
    const int head = s_head, count = s_count, push = s_push, slot = s_slot;
    const double H = s_H;
    const int oldest = (head - count + m) % m;
    if (push) {
        // the new pair's row and column of both blocks (dots against slot `slot` itself were taken with the row it evicts: not read)
        for (int a = tid; a < count; a += 256) {
            const int j = (oldest + a) % m;
            if (j == slot) continue;
            const double* dj = dots + LBFGS_PER_SLOT * j;
            SY[(size_t)j * m + slot] = dj[2];                      // S_j . y
            SY[(size_t)slot * m + j] = dj[3];                      // s . Y_j
            YY[(size_t)j * m + slot] = dj[4]; YY[(size_t)slot * m + j] = dj[4];
        }
        if (tid == 0) { SY[(size_t)slot * m + slot] = dots[B + LBD_YS]; YY[(size_t)slot * m + slot] = dots[B + LBD_YY]; }
        __syncthreads();
        if (tid == 0) { dots[LBFGS_PER_SLOT * slot + 0] = dots[B + LBD_SG]; dots[LBFGS_PER_SLOT * slot + 1] = dots[B + LBD_YG]; }
        __threadfence_block();
        __syncthreads();
    }
    // thread a < count owns the pair of age a (0 = oldest)
    const int ja = tid < count ? (oldest + tid) % m : 0;
    double wa = tid < count ? -dots[LBFGS_PER_SLOT * ja + 0] : 0.0;
    for (int i = count - 1; i >= 0; --i) {                         // al, newest to oldest
        const int ji = (oldest + i) % m;
        if (tid == i) al[i] = ro[ji] * wa;
        __syncthreads();
        if (tid < i) wa -= al[i] * SY[(size_t)ja * m + ji];
    }
    double va = 0.0;
    if (tid < count) {
        double u = -dots[LBFGS_PER_SLOT * ja + 1];
        for (int j = 0; j < count; ++j) u -= al[j] * YY[(size_t)ja * m + (oldest + j) % m];
        va = H * u;
    }
    for (int i = 0; i < count; ++i) {                              // be, oldest to newest; cs = al - be
        const int ji = (oldest + i) % m;
        if (tid == i) cs[i] = al[i] - ro[ji] * va;
        __syncthreads();
        if (tid > i && tid < count) va += cs[i] * SY[(size_t)ji * m + ja];
    }
    __syncthreads();
    for (int j = tid; j < m; j += 256) { coef[j] = 0.0; coef[m + j] = 0.0; }
    __syncthreads();
    if (tid < count) { coef[ja] = cs[tid]; coef[m + ja] = -H * al[tid]; w[tid] = cs[tid] * dots[LBFGS_PER_SLOT * ja + 0] - H * al[tid] * dots[LBFGS_PER_SLOT * ja + 1]; }
    __syncthreads();
    if (tid == 0) {
        const double cg = mode == 1 ? -1.0 : -H;
        coef[2 * m] = cg;
        double gtd = cg * gg;
        for (int a = 0; a < count; ++a) gtd += w[a];
        const double t = mode == 1 ? fmin(1.0, 1.0 / g1) * cfg.lr : cfg.lr;
        const int skip = gtd > -cfg.tol_change;
        st->H_diag = H; st->tick.t_pair = st->t; st->t = t; st->prev_loss = loss; st->n_iter += 1;
        st->head = head; st->count = count; st->tick.push = push; st->tick.push_slot = slot; st->tick.skip = skip;
        lbfgs_record(st, loss, gmax, g1, gtd, skip, push, mode == 2 ? dots[B + LBD_YS] : 0.0);
        if constexpr (LS) ls_rearm(st, loss, gtd, t, skip);
    }
}

// one element of the iteration: the pushed pair into the rings, d = sum_j c_j b_j over the live slots in fp64, rounded once -> d[i]
GPE_DEV float lbfgs_iterate(int i, int ld, int m, float g, const float* __restrict__ g_prev, float* __restrict__ d, float* __restrict__ S,
                            float* __restrict__ Y, const LbfgsDev* __restrict__ st, const double* __restrict__ coef) {
    const int head = st->head, count = st->count;
    if (st->tick.push) {
        const int slot = st->tick.push_slot;
        S[(size_t)slot * ld + i] = (float)(st->tick.t_pair * (double)d[i]);
        Y[(size_t)slot * ld + i] = g - g_prev[i];
    }
    double acc = coef[2 * m] * (double)g;
    for (int j = 0; j < m; ++j) {
        if (!lbfgs_live(j, head, count, m)) continue;
        acc += coef[j] * (double)S[(size_t)j * ld + i] + coef[m + j] * (double)Y[(size_t)j * ld + i];
    }
    const float dn = (float)acc;
    d[i] = dn;
    return dn;
}

template <bool LS>
__global__ __launch_bounds__(256) void k_lbfgs_apply(int P, int ld, int m, const float* __restrict__ grad, float* __restrict__ g_prev,
                                                      float* __restrict__ d, float* __restrict__ S, float* __restrict__ Y, float* __restrict__ theta,
                                                      const LbfgsDev* __restrict__ st, const double* __restrict__ coef) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if constexpr (LS) {
        // the move.  TRIAL: the next trial; RESTORE: the best point held (the new theta0); ACCEPT: theta0 = that point, the iteration, the first trial
        const int action = st->tick.action;
        if (i >= P || action == LS_ACT_NONE) return;
        float* theta0 = st->ls.theta0;
        if (action == LS_ACT_TRIAL) { theta[i] = ls_point(theta0[i], st->ls.t, d[i]); return; }
        const float th0 = st->tick.from_idle ? theta[i] : ls_point(theta0[i], st->tick.t_acc, d[i]);
        theta0[i] = th0;
        if (action == LS_ACT_RESTORE || st->frozen) { theta[i] = th0; return; }
        const int acc_slot = st->tick.acc_slot;
        const float g = ls_slot_ptr(st, g_prev, ld, acc_slot)[i];
        const float dn = lbfgs_iterate(i, ld, m, g, g_prev, d, S, Y, st, coef);
        if (acc_slot != LS_START_SLOT) g_prev[i] = g;
        theta[i] = st->tick.skip ? th0 : ls_point(th0, st->t, dn);
    } else {
        if (i >= P || st->frozen) return;
        const float g = grad[i];
        const float dn = lbfgs_iterate(i, ld, m, g, g_prev, d, S, Y, st, coef);
        g_prev[i] = g;
        if (!st->tick.skip) theta[i] = (float)((double)theta[i] + st->t * (double)dn);
    }
}

// part[blockIdx.x][LSD_COUNT]: g.d, sum|g|, max|g|, max|d| of this workgroup's tiles; g goes into slot LsDev::slot_new.  Frozen: writes nothing.
__global__ __launch_bounds__(64) void k_ls_dots(int P, int ld, const float* __restrict__ grad, const float* __restrict__ d,
                                                 const LbfgsDev* __restrict__ st, double* __restrict__ part) {
    if (st->frozen) return;
    const int lane = threadIdx.x;
    const int slot = st->ls.slot_new;
    if (slot < 0 || slot >= LS_SLOTS) return;
    float* dst = st->ls.slots + (size_t)slot * ld;
    double gtd = 0.0, g1 = 0.0, gmax = 0.0, dmax = 0.0;
    for (int base = blockIdx.x * LBFGS_TILE; base < P; base += gridDim.x * LBFGS_TILE) {
#pragma unroll
        for (int k = 0; k < LBFGS_E; ++k) {
            const int i = base + k * 64 + lane;
            if (i < P) {
                const float g = grad[i];
                dst[i] = g;
                const double gd = g, dd = d[i];
                gtd += gd * dd; g1 += fabs(gd); gmax = fmax(gmax, fabs(gd)); dmax = fmax(dmax, fabs(dd));
            }
        }
    }
    gtd = lbfgs_wave_sum(gtd); g1 = lbfgs_wave_sum(g1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { gmax = fmax(gmax, __shfl_down(gmax, o, 64)); dmax = fmax(dmax, __shfl_down(dmax, o, 64)); }
    if (lane == 0) {
        double* row = part + (size_t)blockIdx.x * LSD_COUNT;
        row[LSD_GTD] = gtd; row[LSD_G1] = g1; row[LSD_GMAX] = gmax; row[LSD_DMAX] = dmax;
    }
}

// one lane adds the rows in index order and runs ls_decide on the loss the record launch left in `last`
__global__ __launch_bounds__(64) void k_ls_decide(int n_part, LbfgsCfg cfg, LsCfg lc, LbfgsDev* __restrict__ st, const double* __restrict__ part,
                                                   const gpe_scalars* __restrict__ last) {
    if (threadIdx.x != 0) return;
    double gtd_new = 0.0, g1 = 0.0, gmax = 0.0, dmax = 0.0;
    for (int r = 0; r < n_part; ++r) {                             // (stale rows behind a frozen state: ls_decide reads none of it)
        const double* row = part + (size_t)r * LSD_COUNT;
        gtd_new += row[LSD_GTD]; g1 += row[LSD_G1]; gmax = fmax(gmax, row[LSD_GMAX]); dmax = fmax(dmax, row[LSD_DMAX]);
    }
    ls_decide(st, cfg, lc, last->loss, gtd_new, g1, gmax, dmax);
}

// a reset that does not rewrite theta ends a running search: theta goes back to the search's start point first
__global__ __launch_bounds__(256) void k_ls_restore(int P, float* __restrict__ theta, const LbfgsDev* __restrict__ st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P && lbfgs_judged_at_start(st)) theta[i] = st->ls.theta0[i];
}

// ---- the judged point: what the monitor and the keeper see in a gpe_lbfgs_run (gpe_lbfgs_monitor, gpe_lbfgs_point) ---------------------
// While a search runs theta sits at a trial point and the judged point is the search's START point (lbfgs_judged_at_start); else it is
// theta.  k_lbfgs_view, in front of the monitor chain, sets theta aside and puts the start point in its place (LbfgsTick::view says so
// to the kernel behind); k_lbfgs_unview brings theta back -- unless the keeper's patience fired (KeepDev::stopped): then theta stays
// and the run freezes with LBFGS_FROZEN_KEEPER.  Grid-strided, 16 bytes per access where the pointers allow, grid a function of P alone.
#define LBV_THREADS 256
#define LBV_MAX_WG 256
static inline unsigned lbfgs_view_grid(int P) {
    const int g = ((P + 3) / 4 + LBV_THREADS - 1) / LBV_THREADS;
    return (unsigned)(g < 1 ? 1 : g < LBV_MAX_WG ? g : LBV_MAX_WG);
}

// dst = src over P floats; ASIDE: `keep` takes dst's old values first
template <bool ASIDE>
GPE_DEV void lbfgs_view_copy(int P, float* __restrict__ dst, const float* __restrict__ src, float* __restrict__ keep) {
    const bool wide = ((((uintptr_t)dst) | ((uintptr_t)src) | ((uintptr_t)keep)) & 15) == 0;
    const int n4 = wide ? P / 4 : 0;
    float4* d4 = (float4*)dst; const float4* s4 = (const float4*)src; float4* k4 = (float4*)keep;
    for (int i = blockIdx.x * LBV_THREADS + threadIdx.x; i < n4; i += gridDim.x * LBV_THREADS) {
        if constexpr (ASIDE) k4[i] = d4[i];
        d4[i] = s4[i];
    }
    for (int i = 4 * n4 + blockIdx.x * LBV_THREADS + threadIdx.x; i < P; i += gridDim.x * LBV_THREADS) {
        if constexpr (ASIDE) keep[i] = dst[i];
        dst[i] = src[i];
    }
}

__global__ __launch_bounds__(LBV_THREADS) void k_lbfgs_view(int P, float* __restrict__ theta, float* __restrict__ aside, LbfgsDev* st) {
    const bool at_start = lbfgs_judged_at_start(st);                // (no thread writes a field this reads)
    if (blockIdx.x == 0 && threadIdx.x == 0) st->tick.view = at_start ? 1 : 0;
    if (!at_start) return;
    lbfgs_view_copy<true>(P, theta, st->ls.theta0, aside);
}

// kd == NULL: no keeper bound
__global__ __launch_bounds__(LBV_THREADS) void k_lbfgs_unview(int P, float* __restrict__ theta, const float* __restrict__ aside, LbfgsDev* st,
                                                               const KeepDev* __restrict__ kd) {
    const bool stop = kd != nullptr && kd->stopped != 0;
    const bool viewed = st->tick.view != 0;                              // (written by k_lbfgs_view only)
    if (blockIdx.x == 0 && threadIdx.x == 0 && stop && !st->frozen)       // `frozen` is read and written by this thread alone
        lbfgs_freeze(st, LBFGS_FROZEN_KEEPER, st->ls.theta0 != nullptr);     // (the line search's buffers exist: its record is read)
    if (!viewed || stop) return;                                    // a viewed state is never a frozen one: `stop` freezes it here
    lbfgs_view_copy<false>(P, theta, aside, nullptr);
}
