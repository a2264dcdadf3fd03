// gpe_lbfgs.h -- one L-BFGS iteration on the device, as torch.optim.LBFGS without a line search takes it (the reference's
// pretrain_on_analytical_solution tail, refine/harmonic_pinn_simulation.py:672-687, and its 2D hybrid driver).  Without a line search
// torch's outer / inner loop is a flat sequence "evaluate, iterate" (tests/lbfgs_ref.py holds that restatement to torch in fp64), so an
// iteration is three launches behind the evaluation's gradient and record:
//   k_lbfgs_dots    y = g - g_prev and s = t d formed on the fly (both rounded to fp32, as the rings will hold them); their dot products
//                   with every live ring row and those of g with every live row, y.y, y.s, s.g, y.g, g.g, sum|g|, max|g|.  One wave per
//                   workgroup, grid a function of P alone, element -> lane map fixed, fp64 accumulation, one fp64 partial row per
//                   workgroup, no atomics: the result is the same bits on every run (the discipline of k_obs_pass1 / k_grad_reduce).
//   k_lbfgs_coef    one workgroup: adds the partial rows in index order; torch's rules (push only if ys > 1e-10, pop the oldest at
//                   `history`, H_diag = ys / yy, d = -g and t = min(1, 1/|g|_1) lr on the first iteration, t = lr after it, no update if
//                   g.d > -tolerance_change); freezes for good on max|g| <= tolerance_grad, a non-finite loss or gradient, or
//                   loss < stop_loss (when stop_loss > 0); updates the Gram blocks; runs the two-loop recursion on COEFFICIENTS in fp64 and leaves the
//                   coefficients of d over the basis {S_j, Y_j, g} and the record.
//   k_lbfgs_apply   commits the pushed pair into the rings, d = sum_j c_j b_j accumulated per element in fp64 and rounded once,
//                   g_prev = g, theta += t d (formed in fp64, rounded once).  A frozen iteration writes nothing; a skipped one writes
//                   everything but theta.
// The two-loop recursion over VECTORS is 2m dependent reductions over P; over coefficients it is one pass of independent dot products,
// an O(m^2) scalar recursion and one combination pass.  With the pairs in age order 0 (oldest) .. n-1, q = -g - sum_j al_j Y_j and
// r = H q + sum_j (al_j - be_j) S_j give
//   al_i = ro_i (-S_i.g - sum_{j > i} al_j S_i.Y_j)                        newest to oldest
//   u_i  = Y_i.q = -Y_i.g - sum_j al_j Y_i.Y_j
//   be_i = ro_i (H u_i + sum_{j < i} (al_j - be_j) S_j.Y_i)                oldest to newest
//   d    = -H g - H sum_j al_j Y_j + sum_j (al_j - be_j) S_j
// so the recursion reads the blocks S.Y (m x m, not symmetric) and Y.Y (symmetric) and the row of g; S.S is never read and not kept.
// Ring rows live in PHYSICAL slots (a push overwrites one row and one row / column of each block); `head` is the slot of the next push,
// the live slots are head - count .. head - 1 (mod m).
#pragma once

#define LBFGS_MAX_HISTORY 128
#define LBFGS_E 8                               // elements per lane and tile
#define LBFGS_TILE (64 * LBFGS_E)
#define LBFGS_MAX_WG 128
#define LBFGS_PER_SLOT 5                        // S_j.g, Y_j.g, S_j.y, s.Y_j, y.Y_j
enum { LBD_YS = 0, LBD_YY, LBD_SG, LBD_YG, LBD_GG, LBD_G1, LBD_GMAX, LBD_BASE_COUNT = 8 };
enum { LBR_LOSS = 0, LBR_GMAX, LBR_G1, LBR_T, LBR_GTD, LBR_N_ITER, LBR_COUNT, LBR_FROZEN, LBR_SKIPPED, LBR_PUSHED, LBR_YS, LBR_H_DIAG,
       LBR_HEAD, LBR_PREV_LOSS, LBR_FIELDS = 16 };
enum { LBFGS_LIVE = 0, LBFGS_FROZEN_GRAD = 1, LBFGS_FROZEN_NONFINITE = 2, LBFGS_FROZEN_LOSS = 3 };

struct LbfgsCfg { double lr, tol_grad, tol_change, stop_loss; int m; };
struct LbfgsDev {
    double H_diag, t, t_pair, prev_loss;        // t: step of the LAST iteration (s = t d of the next pair; kept in t_pair for k_lbfgs_apply)
    long long n_iter;
    int head, count, frozen;
    int push, push_slot, skip;                  // this iteration's decisions, for k_lbfgs_apply
    double rec[LBR_FIELDS];
};

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

__global__ __launch_bounds__(64) void k_lbfgs_dots(int P, int ld, int m, const float* __restrict__ grad, const float* __restrict__ g_prev,
                                                    const float* __restrict__ d, const float* __restrict__ S, const float* __restrict__ Y,
                                                    const LbfgsDev* __restrict__ st, double* __restrict__ part) {
    __shared__ double acc[LBFGS_PER_SLOT * LBFGS_MAX_HISTORY + LBD_BASE_COUNT];
    const int lane = threadIdx.x, W = LBFGS_PER_SLOT * m + LBD_BASE_COUNT;
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

// SY[a * m + b] = S_a . Y_b, YY[a * m + b] = Y_a . Y_b over physical slots; coef = [cS (m) | cY (m) | c_g]
__global__ __launch_bounds__(256) void k_lbfgs_coef(int m, int n_part, LbfgsCfg cfg, LbfgsDev* __restrict__ st, const double* __restrict__ part,
                                                     double* __restrict__ SY, double* __restrict__ YY, double* __restrict__ ro,
                                                     double* __restrict__ coef, const gpe_scalars* __restrict__ last) {
    __shared__ double dots[LBFGS_PER_SLOT * LBFGS_MAX_HISTORY + LBD_BASE_COUNT];
    __shared__ double al[LBFGS_MAX_HISTORY], cs[LBFGS_MAX_HISTORY], w[LBFGS_MAX_HISTORY];
    __shared__ int s_mode, s_head, s_count, s_push, s_slot;
    __shared__ double s_H;
    const int tid = threadIdx.x, W = LBFGS_PER_SLOT * m + LBD_BASE_COUNT, B = LBFGS_PER_SLOT * m;
    for (int v = tid; v < W; v += 256) {
        double a = 0.0;
        if (v == B + LBD_GMAX) { for (int r = 0; r < n_part; ++r) a = fmax(a, part[(size_t)r * W + v]); }
        else { for (int r = 0; r < n_part; ++r) a += part[(size_t)r * W + v]; }
        dots[v] = a;
    }
    __syncthreads();
    const double loss = last->loss, g1 = dots[B + LBD_G1], gmax = dots[B + LBD_GMAX], gg = dots[B + LBD_GG];
    if (tid == 0) {
        int frozen = st->frozen;
        if (!frozen) {
            if (!(isfinite(loss) && isfinite(g1))) frozen = LBFGS_FROZEN_NONFINITE;
            else if (gmax <= cfg.tol_grad) frozen = LBFGS_FROZEN_GRAD;
            else if (cfg.stop_loss > 0.0 && loss < cfg.stop_loss) frozen = LBFGS_FROZEN_LOSS;      // (0: no such stop)
        }
        int head = st->head, count = st->count, push = 0, slot = 0, mode = 0;      // mode: 0 frozen, 1 first iteration, 2 later
        double H = st->H_diag;
        if (frozen) {
            st->frozen = frozen; st->push = 0; st->skip = 1;
            double* r = st->rec;
            r[LBR_LOSS] = loss; r[LBR_GMAX] = gmax; r[LBR_G1] = g1; r[LBR_T] = st->t; r[LBR_GTD] = 0.0; r[LBR_N_ITER] = (double)st->n_iter;
            r[LBR_COUNT] = count; r[LBR_FROZEN] = frozen; r[LBR_SKIPPED] = 1.0; r[LBR_PUSHED] = 0.0; r[LBR_YS] = 0.0; r[LBR_H_DIAG] = H;
            r[LBR_HEAD] = head; r[LBR_PREV_LOSS] = st->prev_loss;
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
        const double t_old = st->t;
        const double t = mode == 1 ? fmin(1.0, 1.0 / g1) * cfg.lr : cfg.lr;
        const int skip = gtd > -cfg.tol_change;
        const long long n_iter = st->n_iter + 1;
        st->H_diag = H; st->t_pair = t_old; st->t = t; st->prev_loss = loss; st->n_iter = n_iter;
        st->head = head; st->count = count; st->push = push; st->push_slot = slot; st->skip = skip;
        double* r = st->rec;
        r[LBR_LOSS] = loss; r[LBR_GMAX] = gmax; r[LBR_G1] = g1; r[LBR_T] = t; r[LBR_GTD] = gtd; r[LBR_N_ITER] = (double)n_iter;
        r[LBR_COUNT] = count; r[LBR_FROZEN] = 0.0; r[LBR_SKIPPED] = skip; r[LBR_PUSHED] = push; r[LBR_YS] = mode == 2 ? dots[B + LBD_YS] : 0.0;
        r[LBR_H_DIAG] = H; r[LBR_HEAD] = head; r[LBR_PREV_LOSS] = loss;
    }
}

__global__ __launch_bounds__(256) void k_lbfgs_apply(int P, int ld, int m, const float* __restrict__ grad, float* __restrict__ g_prev,
                                                      float* __restrict__ d, float* __restrict__ S, float* __restrict__ Y,
                                                      float* __restrict__ theta, const LbfgsDev* __restrict__ st,
                                                      const double* __restrict__ coef) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || st->frozen) return;
    const float g = grad[i];
    const int head = st->head, count = st->count;
    if (st->push) {
        const int slot = st->push_slot;
        S[(size_t)slot * ld + i] = (float)(st->t_pair * (double)d[i]);
        Y[(size_t)slot * ld + i] = g - g_prev[i];
    }
    double acc = coef[2 * m] * (double)g;
    for (int j = 0; j < m; ++j) {
        if (!lbfgs_live(j, head, count, m)) continue;
        acc += coef[j] * (double)S[(size_t)j * ld + i] + coef[m + j] * (double)Y[(size_t)j * ld + i];
    }
    const float dn = (float)acc;
    d[i] = dn;
    g_prev[i] = g;
    if (!st->skip) theta[i] = (float)((double)theta[i] + st->t * (double)dn);
}
