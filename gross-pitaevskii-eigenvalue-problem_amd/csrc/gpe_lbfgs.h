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
//
// Strong-Wolfe line search (gpe_lbfgs_line_search; torch's `_strong_wolfe`, flattened: tests/lbfgs_ls_ref.py holds the restatement to torch).
// With it the flat sequence is "evaluate, tick": a tick is a line-search decision, followed by the iteration above only if the decision
// ACCEPTS a point.  Every tick is the same five launches behind the evaluation's record, and the host never reads a decision:
//   k_ls_dots       reads the new gradient once, writes it into the free one of three trial-gradient slots and forms g.d, sum|g|, max|g|
//                   and max|d| (same discipline as k_lbfgs_dots: one fp64 partial row per workgroup, no atomics).
//   k_ls_decide     one wave: adds the rows in index order and runs the state machine on the recorded loss: the next trial step t, or
//                   accept(slot, t, loss), or -- a non-finite loss or gradient at a trial -- back to the best point held and frozen (2).
//   k_lbfgs_dots<true>, k_lbfgs_coef<true>, k_lbfgs_apply<true>
//                   the iteration on the ACCEPTED slot's gradient and loss (the accepted point need not be the last one evaluated); they
//                   return at once, on a grid-uniform branch on LsDev::action, when the tick did not accept.  k_lbfgs_apply<true> also
//                   carries the move: theta = fl32(theta0 + t d) in fp64, rounded once; on accept theta0 = fl32(theta0 + t_acc d) first
//                   (the bits the accepted gradient was evaluated at), then the first trial of the new direction.
// Gradients are referred to BY SLOT INDEX in the state (0..2 trial slots, 3 = g_prev, the gradient at theta0); none is ever copied between
// slots: at most two bracket ends and the new point are live.  The <false> instantiations are the kernels as they were.
#pragma once

#define LBFGS_MAX_HISTORY 128
#define LBFGS_E 8                               // elements per lane and tile
#define LBFGS_TILE (64 * LBFGS_E)
#define LBFGS_MAX_WG 128
#define LBFGS_PER_SLOT 5                        // S_j.g, Y_j.g, S_j.y, s.Y_j, y.Y_j
enum { LBD_YS = 0, LBD_YY, LBD_SG, LBD_YG, LBD_GG, LBD_G1, LBD_GMAX, LBD_BASE_COUNT = 8 };
enum { LBR_LOSS = 0, LBR_GMAX, LBR_G1, LBR_T, LBR_GTD, LBR_N_ITER, LBR_COUNT, LBR_FROZEN, LBR_SKIPPED, LBR_PUSHED, LBR_YS, LBR_H_DIAG,
       LBR_HEAD, LBR_PREV_LOSS, LBR_FIELDS = 16 };
enum { LBFGS_LIVE = 0, LBFGS_FROZEN_GRAD = 1, LBFGS_FROZEN_NONFINITE = 2, LBFGS_FROZEN_LOSS = 3, LBFGS_FROZEN_KEEPER = 4 };

// line search: what the NEXT evaluation is for / what this tick's decision asks of the kernels behind it / what the tick did (the record)
enum { LS_IDLE = 0, LS_BRACKET = 1, LS_ZOOM = 2 };      // IDLE: taken at theta0 itself (the first one, or the one after a g.d skip)
enum { LS_ACT_NONE = 0, LS_ACT_TRIAL = 1, LS_ACT_ACCEPT = 2, LS_ACT_RESTORE = 3 };
enum { LS_DID_NONE = 0, LS_DID_BRACKET = 1, LS_DID_ZOOM = 2, LS_DID_ACCEPTED = 3, LS_DID_FROZEN = 4 };
enum { LS_START_SLOT = 3, LS_SLOTS = 3 };
enum { LSD_GTD = 0, LSD_G1, LSD_GMAX, LSD_DMAX, LSD_COUNT };
enum { LSR_PHASE = 0, LSR_LS_ITER, LSR_LS_EVALS, LSR_EVALS_TOTAL, LSR_T, LSR_T_PREV, LSR_B0, LSR_B1, LSR_BF0, LSR_BF1, LSR_BGTD0, LSR_BGTD1,
       LSR_LOW_POS, LSR_F0, LSR_GTD0, LSR_DNORM, LSR_ACCEPTED, LSR_END_MAX_LS, LSR_END_WIDTH, LSR_END_CURV, LSR_STALLED, LSR_INSUF,
       LSR_BSLOTS, LSR_SLOT_NEW, LSR_FIELDS = 24 };
struct LsCfg { int kind; double c1, c2; int max_ls; };
struct LsDev {
    float *slots, *theta0;                      // [3][ld] trial gradients, [ld] the search's start point (set by the host at every reset)
    double t, t_acc, f_acc, gtd_acc, f0, gtd0, dnorm;      // t: the step of the trial being evaluated
    double b[2], bf[2], bgtd[2];                // bracket ends; in LS_BRACKET end 0 is the previous trial (t_prev) and end 1, until a
                                                // bracket forms, the point the previous search accepted (step, loss, g.d along the old d)
    int bslot[2];                               // gradient slot per end
    int state, action, did, from_idle, acc_slot, slot_new, low_pos, insuf, ls_iter, ls_evals;
    long long evals_total, accepted, end_max_ls, end_width, end_curv, stalled;
};

struct LbfgsCfg { double lr, tol_grad, tol_change, stop_loss; int m; };
struct LbfgsDev {
    double H_diag, t, t_pair, prev_loss;        // t: step of the LAST iteration (s = t d of the next pair; kept in t_pair for k_lbfgs_apply)
    long long n_iter;
    int head, count, frozen;
    int push, push_slot, skip;                  // this iteration's decisions, for k_lbfgs_apply
    double rec[LBR_FIELDS];
    LsDev ls;                                   // all zero with the line search off
    int view;                                   // k_lbfgs_view put the search's start point in theta's place (until k_lbfgs_unview)
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
        if (st->ls.action != LS_ACT_ACCEPT) return;
        grad = ls_slot_ptr(st, g_prev, ld, st->ls.acc_slot);
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
    if constexpr (LS) { if (st->ls.action != LS_ACT_ACCEPT) return; }
    for (int v = tid; v < W; v += 256) {
        double a = 0.0;
        if (v == B + LBD_GMAX) { for (int r = 0; r < n_part; ++r) a = fmax(a, part[(size_t)r * W + v]); }
        else { for (int r = 0; r < n_part; ++r) a += part[(size_t)r * W + v]; }
        dots[v] = a;
    }
    __syncthreads();
    const double loss = LS ? st->ls.f_acc : last->loss, g1 = dots[B + LBD_G1], gmax = dots[B + LBD_GMAX], gg = dots[B + LBD_GG];
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
            if constexpr (LS) { st->ls.state = LS_IDLE; st->ls.did = LS_DID_FROZEN; }      // (k_lbfgs_apply<true> leaves theta at the accepted point)
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
        if constexpr (LS) {                                         // the search along the new direction starts at the accepted point
            LsDev& ls = st->ls;
            ls.f0 = loss; ls.gtd0 = gtd; ls.t = t;
            ls.b[0] = 0.0; ls.bf[0] = loss; ls.bgtd[0] = gtd; ls.bslot[0] = LS_START_SLOT;
            ls.b[1] = ls.t_acc; ls.bf[1] = loss; ls.bgtd[1] = ls.gtd_acc; ls.bslot[1] = LS_START_SLOT;
            ls.low_pos = 0; ls.insuf = 0; ls.ls_iter = 0; ls.ls_evals = 0; ls.slot_new = 0;
            ls.state = skip ? LS_IDLE : LS_BRACKET; ls.did = LS_DID_ACCEPTED;
        }
    }
}

template <bool LS>
__global__ __launch_bounds__(256) void k_lbfgs_apply(int P, int ld, int m, const float* __restrict__ grad, float* __restrict__ g_prev,
                                                      float* __restrict__ d, float* __restrict__ S, float* __restrict__ Y,
                                                      float* __restrict__ theta, const LbfgsDev* __restrict__ st,
                                                      const double* __restrict__ coef) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if constexpr (LS) {
        // the tick's move.  TRIAL: the next trial point; RESTORE: back to the best point held (and it becomes the start point);
        // ACCEPT: the accepted point becomes the start point, then the iteration below and the first trial of the new direction
        const int action = st->ls.action;
        if (i >= P || action == LS_ACT_NONE) return;
        float* theta0 = st->ls.theta0;
        if (action == LS_ACT_TRIAL) { theta[i] = ls_point(theta0[i], st->ls.t, d[i]); return; }
        const float th0 = st->ls.from_idle ? theta[i] : ls_point(theta0[i], st->ls.t_acc, d[i]);
        theta0[i] = th0;
        if (action == LS_ACT_RESTORE || st->frozen) { theta[i] = th0; return; }
        const int acc_slot = st->ls.acc_slot;
        const float g = ls_slot_ptr(st, g_prev, ld, acc_slot)[i];
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
        if (acc_slot != LS_START_SLOT) g_prev[i] = g;
        theta[i] = st->skip ? th0 : ls_point(th0, st->t, dn);
        return;
    }
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

// ---- strong-Wolfe line search ----------------------------------------------------------------------------------------------------------
// part[blockIdx.x][LSD_COUNT]: g.d, sum|g|, max|g|, max|d| of this workgroup's tiles; the gradient goes into slot LsDev::slot_new.
// A frozen state: nothing is written.
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

// torch.optim.lbfgs._cubic_interpolate; bounded: the bracket phase's (min_step, max_step), else the ends
GPE_DEV double ls_cubic(double x1, double f1, double g1, double x2, double f2, double g2, bool bounded, double lo, double hi) {
    if (!bounded) { lo = x1 <= x2 ? x1 : x2; hi = x1 <= x2 ? x2 : x1; }
    const double d1 = g1 + g2 - 3.0 * (f1 - f2) / (x1 - x2);
    const double d2_square = d1 * d1 - g1 * g2;
    if (d2_square >= 0.0) {
        const double d2 = sqrt(d2_square);
        const double min_pos = x1 <= x2 ? x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2.0 * d2))
                                        : x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2.0 * d2));
        // python's min(max(min_pos, lo), hi): a NaN min_pos stays (max(nan, lo) = nan there; min(nan, hi) = nan)
        const double a = lo > min_pos ? lo : min_pos;
        return hi < a ? hi : a;
    }
    return (lo + hi) / 2.0;
}

GPE_DEV void ls_accept(LbfgsDev* st, double t_acc, double f_acc, double gtd_acc, int slot) {
    LsDev& ls = st->ls;
    ls.action = LS_ACT_ACCEPT; ls.from_idle = 0; ls.t_acc = t_acc; ls.f_acc = f_acc; ls.gtd_acc = gtd_acc; ls.acc_slot = slot;
    ls.accepted += 1;
    if (t_acc == 0.0) ls.stalled += 1;
    st->t = t_acc;                                                  // s = t_acc d: the pair of the iteration that follows
}
GPE_DEV int ls_free_slot(int a, int b) {
    for (int s = 0; s < LS_SLOTS; ++s) if (s != a && s != b) return s;
    return 0;
}

// One wave; lane 0 adds the partial rows in index order and runs the state machine of tests/lbfgs_ls_ref.py (torch's order of tests) on
// the loss the record launch left in `last`.
__global__ __launch_bounds__(64) void k_ls_decide(int n_part, LbfgsCfg cfg, LsCfg lc, LbfgsDev* __restrict__ st, const double* __restrict__ part,
                                                   const gpe_scalars* __restrict__ last) {
    if (threadIdx.x != 0) return;
    LsDev& ls = st->ls;
    if (st->frozen) { ls.action = LS_ACT_NONE; return; }
    double gtd_new = 0.0, g1 = 0.0, gmax = 0.0, dmax = 0.0;
    for (int r = 0; r < n_part; ++r) {
        const double* row = part + (size_t)r * LSD_COUNT;
        gtd_new += row[LSD_GTD]; g1 += row[LSD_G1]; gmax = fmax(gmax, row[LSD_GMAX]); dmax = fmax(dmax, row[LSD_DMAX]);
    }
    const double loss = last->loss;
    const int slot = ls.slot_new;
    ls.evals_total += 1;
    if (ls.state == LS_IDLE) {                                      // an evaluation at theta0: the iteration's own rules decide
        ls.action = LS_ACT_ACCEPT; ls.from_idle = 1; ls.t_acc = 0.0; ls.f_acc = loss; ls.gtd_acc = 0.0; ls.acc_slot = slot;
        return;
    }
    if (ls.ls_evals == 0) ls.dnorm = dmax;
    ls.ls_evals += 1;
    if (!(isfinite(loss) && isfinite(g1))) {                        // never leave theta at such a trial
        ls.action = LS_ACT_RESTORE; ls.from_idle = 0;
        ls.t_acc = ls.state == LS_ZOOM ? ls.b[ls.low_pos] : 0.0;
        ls.state = LS_IDLE; ls.did = LS_DID_FROZEN;
        st->frozen = LBFGS_FROZEN_NONFINITE;
        st->rec[LBR_FROZEN] = LBFGS_FROZEN_NONFINITE;
        return;
    }
    const double t = ls.t, f0 = ls.f0, gtd0 = ls.gtd0;
    double* b = ls.b; double* bf = ls.bf; double* bgtd = ls.bgtd; int* bslot = ls.bslot;
    bool done = false;
    if (ls.state == LS_BRACKET) {
        if (ls.ls_iter < lc.max_ls) {
            bool to_zoom = loss > f0 + lc.c1 * t * gtd0 || (ls.ls_iter > 1 && loss >= bf[0]);
            if (!to_zoom) {
                if (fabs(gtd_new) <= -lc.c2 * gtd0) { ls.end_curv += 1; ls_accept(st, t, loss, gtd_new, slot); return; }
                to_zoom = gtd_new >= 0.0;
            }
            if (!to_zoom) {                                         // extrapolate
                const double t_next = ls_cubic(b[0], bf[0], bgtd[0], t, loss, gtd_new, true, t + 0.01 * (t - b[0]), t * 10.0);
                b[0] = t; bf[0] = loss; bgtd[0] = gtd_new; bslot[0] = slot;
                ls.ls_iter += 1; ls.t = t_next; ls.slot_new = ls_free_slot(slot, slot);
                ls.action = LS_ACT_TRIAL; ls.did = LS_DID_BRACKET;
                return;
            }
        } else {                                                    // torch's fallback at max_ls: the bracket [0, t]
            b[0] = 0.0; bf[0] = f0; bgtd[0] = gtd0; bslot[0] = LS_START_SLOT;
        }
        b[1] = t; bf[1] = loss; bgtd[1] = gtd_new; bslot[1] = slot;
        ls.insuf = 0;
        ls.low_pos = bf[0] <= bf[1] ? 0 : 1;
    } else {
        ls.ls_iter += 1;
        const int low = ls.low_pos, high = 1 - low;
        if (loss > f0 + lc.c1 * t * gtd0 || loss >= bf[low]) {
            b[high] = t; bf[high] = loss; bgtd[high] = gtd_new; bslot[high] = slot;
            ls.low_pos = bf[0] <= bf[1] ? 0 : 1;
        } else {
            if (fabs(gtd_new) <= -lc.c2 * gtd0) done = true;
            else if (gtd_new * (b[high] - b[low]) >= 0.0) { b[high] = b[low]; bf[high] = bf[low]; bgtd[high] = bgtd[low]; bslot[high] = bslot[low]; }
            b[low] = t; bf[low] = loss; bgtd[low] = gtd_new; bslot[low] = slot;
        }
    }
    // the head of torch's zoom loop
    const int low = ls.low_pos;
    if (done) { ls.end_curv += 1; ls_accept(st, b[low], bf[low], bgtd[low], bslot[low]); return; }
    if (ls.ls_iter >= lc.max_ls) { ls.end_max_ls += 1; ls_accept(st, b[low], bf[low], bgtd[low], bslot[low]); return; }
    if (fabs(b[1] - b[0]) * ls.dnorm < cfg.tol_change) { ls.end_width += 1; ls_accept(st, b[low], bf[low], bgtd[low], bslot[low]); return; }
    double tn = ls_cubic(b[0], bf[0], bgtd[0], b[1], bf[1], bgtd[1], false, 0.0, 0.0);
    const double bmax = b[0] > b[1] ? b[0] : b[1], bmin = b[0] < b[1] ? b[0] : b[1];
    const double eps = 0.1 * (bmax - bmin);
    const double near = (bmax - tn) < (tn - bmin) ? (bmax - tn) : (tn - bmin);
    if (near < eps) {
        if (ls.insuf || tn >= bmax || tn <= bmin) {
            tn = fabs(tn - bmax) < fabs(tn - bmin) ? bmax - eps : bmin + eps;
            ls.insuf = 0;
        } else ls.insuf = 1;
    } else ls.insuf = 0;
    ls.t = tn; ls.state = LS_ZOOM; ls.slot_new = ls_free_slot(bslot[0], bslot[1]);
    ls.action = LS_ACT_TRIAL; ls.did = LS_DID_ZOOM;
}

// a reset that does not rewrite theta ends a running search: theta goes back to the search's start point first
__global__ __launch_bounds__(256) void k_ls_restore(int P, float* __restrict__ theta, const LbfgsDev* __restrict__ st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || st->frozen || st->ls.state == LS_IDLE || !st->ls.theta0) return;
    theta[i] = st->ls.theta0[i];
}

// ---- the judged point: what the held-out monitor and the keeper look at in a gpe_lbfgs_run (gpe_lbfgs_monitor, gpe_lbfgs_point) -----------
// While a strong-Wolfe search runs theta sits at a trial point; the one parameter set an observer may see is the search's START point
// (LsDev::theta0: the last accepted point, or where the run started).  Without a line search, with the search idle (the evaluation is
// taken at theta0 itself) and in every frozen state theta is that point already.  The choice is read from the state on the device:
//   k_lbfgs_view    in front of the monitor chain: theta is set aside and the start point takes its place where the rule says so; the
//                   choice is filed in LbfgsDev::view for the kernel behind the chain (which must not read what it rewrites)
//   k_lbfgs_unview  behind the chain: theta comes back -- unless the keeper's patience fired (KeepDev::stopped, k_keep_decide): then theta
//                   stays at the judged point, a running search is ended and the run freezes for good with code LBFGS_FROZEN_KEEPER
// Both are grid-strided over P, 16 bytes per access where the three pointers allow it (as k_keep_copy), grid a function of P alone.
#define LBV_THREADS 256
#define LBV_MAX_WG 256
static inline unsigned lbfgs_view_grid(int P) {
    const int g = ((P + 3) / 4 + LBV_THREADS - 1) / LBV_THREADS;
    return (unsigned)(g < 1 ? 1 : g < LBV_MAX_WG ? g : LBV_MAX_WG);
}
GPE_DEV bool lbfgs_judged_at_start(const LbfgsDev* st) { return !st->frozen && st->ls.state != LS_IDLE && st->ls.theta0 != nullptr; }

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
    if (blockIdx.x == 0 && threadIdx.x == 0) st->view = at_start ? 1 : 0;
    if (!at_start) return;
    lbfgs_view_copy<true>(P, theta, st->ls.theta0, aside);
}

// kd == NULL: no keeper bound
__global__ __launch_bounds__(LBV_THREADS) void k_lbfgs_unview(int P, float* __restrict__ theta, const float* __restrict__ aside, LbfgsDev* st,
                                                               const KeepDev* __restrict__ kd) {
    const bool stop = kd != nullptr && kd->stopped != 0;
    const bool viewed = st->view != 0;                              // (written by k_lbfgs_view only)
    if (blockIdx.x == 0 && threadIdx.x == 0 && stop && !st->frozen) {      // `frozen` is read and written by this thread alone
        st->frozen = LBFGS_FROZEN_KEEPER; st->push = 0; st->skip = 1;
        st->rec[LBR_FROZEN] = LBFGS_FROZEN_KEEPER;
        if (st->ls.theta0) { st->ls.state = LS_IDLE; st->ls.action = LS_ACT_NONE; st->ls.did = LS_DID_FROZEN; }
    }
    if (!viewed || stop) return;                                    // a viewed state is never a frozen one: `stop` freezes it here
    lbfgs_view_copy<false>(P, theta, aside, nullptr);
}
