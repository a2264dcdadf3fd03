// gpe_lbfgs_rules.h -- the state of the device-resident L-BFGS (gpe_lbfgs.h) and its scalar fp64 rules: the freeze, the judged point and
// the strong-Wolfe state machine (tests/lbfgs_ls_ref.py, whose operand order every expression keeps).  No HIP here: one lane of a kernel
// calls these, the host calls lbfgs_judged_at_start, and tests/lbfgs_rules_selftest.cpp compiles the file alone under the host sanitizers.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define LBFGS_RULE __host__ __device__ __forceinline__
#else
#define LBFGS_RULE static inline
#endif

#define LBFGS_MAX_HISTORY 128
enum { LBR_LOSS = 0, LBR_GMAX, LBR_G1, LBR_T, LBR_GTD, LBR_N_ITER, LBR_COUNT, LBR_FROZEN, LBR_SKIPPED, LBR_PUSHED, LBR_YS, LBR_H_DIAG,
       LBR_HEAD, LBR_PREV_LOSS, LBR_FIELDS = 16 };
enum { LBFGS_LIVE = 0, LBFGS_FROZEN_GRAD = 1, LBFGS_FROZEN_NONFINITE = 2, LBFGS_FROZEN_LOSS = 3, LBFGS_FROZEN_KEEPER = 4 };

// line search: what the NEXT evaluation is for / what this tick's decision asks of the kernels behind it / what the tick did (the record)
enum { LS_IDLE = 0, LS_BRACKET = 1, LS_ZOOM = 2 };      // IDLE: taken at theta0 itself (the first one, or the one after a g.d skip)
enum { LS_ACT_NONE = 0, LS_ACT_TRIAL = 1, LS_ACT_ACCEPT = 2, LS_ACT_RESTORE = 3 };
enum { LS_DID_NONE = 0, LS_DID_BRACKET = 1, LS_DID_ZOOM = 2, LS_DID_ACCEPTED = 3, LS_DID_FROZEN = 4 };
enum { LS_START_SLOT = 3, LS_SLOTS = 3 };
enum { LSR_PHASE = 0, LSR_LS_ITER, LSR_LS_EVALS, LSR_EVALS_TOTAL, LSR_T, LSR_T_PREV, LSR_B0, LSR_B1, LSR_BF0, LSR_BF1, LSR_BGTD0, LSR_BGTD1,
       LSR_LOW_POS, LSR_F0, LSR_GTD0, LSR_DNORM, LSR_ACCEPTED, LSR_END_MAX_LS, LSR_END_WIDTH, LSR_END_CURV, LSR_STALLED, LSR_INSUF,
       LSR_BSLOTS, LSR_SLOT_NEW, LSR_FIELDS = 24 };

struct LbfgsCfg { double lr, tol_grad, tol_change, stop_loss; int m; };
struct LsCfg { int kind; double c1, c2; int max_ls; };

// Gradients are referred to BY SLOT INDEX (0..2 trial slots, 3 = g_prev, the gradient at theta0) and never copied between slots
struct LsDev {
    float *slots, *theta0;                      // [3][ld] trial gradients, [ld] the search's start point (set by the host at every reset)
    double t, f0, gtd0, dnorm;                  // t: the step of the trial being evaluated
    double b[2], bf[2], bgtd[2];                // bracket ends; in LS_BRACKET end 0 is the previous trial, end 1 what the last search accepted
    int bslot[2];                               // gradient slot per end
    int state, did, slot_new, low_pos, insuf, ls_iter, ls_evals;
    long long evals_total, accepted, end_max_ls, end_width, end_curv, stalled;
};

// One tick's decisions: read by the kernels BEHIND their writer in the same tick, by no later tick and no reader.   field: writer -> readers
//   action, from_idle, acc_slot, f_acc   ls_decide -> k_lbfgs_dots<true>, k_lbfgs_coef<true>, k_lbfgs_apply<true>
//   t_acc, gtd_acc                       ls_decide -> k_lbfgs_apply<true> (the accepted point), ls_rearm (bracket end 1 of the next search)
//   push, push_slot, skip, t_pair        k_lbfgs_coef (live iterations only) -> k_lbfgs_apply, which asks `frozen` first
//   view                                 k_lbfgs_view -> k_lbfgs_unview
struct LbfgsTick {
    double t_pair, t_acc, f_acc, gtd_acc;       // t_pair: the step of the pair being pushed (LbfgsDev::t is the next step by then)
    int push, push_slot, skip, view, action, from_idle, acc_slot;
};

struct LbfgsDev {
    double H_diag, t, prev_loss;                // t: step of the LAST iteration (s = t d of the next pair)
    long long n_iter;
    int head, count, frozen;
    double rec[LBR_FIELDS];
    LsDev ls;                                   // all zero with the line search off
    LbfgsTick tick;
};

// The run freezes for good (until a reset).  ls_record: a line search takes part in the run, its record reads "frozen" too
// (gpe_lbfgs_ls_read shows it).  LbfgsDev::tick is left alone: what the tick asked of the kernels behind it still holds.
LBFGS_RULE void lbfgs_freeze(LbfgsDev* st, int code, bool ls_record) {
    st->frozen = code; st->rec[LBR_FROZEN] = code;
    if (ls_record) { st->ls.state = LS_IDLE; st->ls.did = LS_DID_FROZEN; }
}

// the judged point (gpe_lbfgs.h) is the running search's start point, not theta
LBFGS_RULE bool lbfgs_judged_at_start(const LbfgsDev* st) { return !st->frozen && st->ls.state != LS_IDLE && st->ls.theta0 != nullptr; }

// torch.optim.lbfgs._cubic_interpolate; bounded: the bracket phase's (min_step, max_step), else the ends
LBFGS_RULE double ls_cubic(double x1, double f1, double g1, double x2, double f2, double g2, bool bounded, double lo, double hi) {
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

LBFGS_RULE int ls_free_slot(int a, int b) {
    for (int s = 0; s < LS_SLOTS; ++s) if (s != a && s != b) return s;
    return 0;
}

// the tick ends a search on the point (t_acc, f_acc, gtd_acc) whose gradient sits in `slot`: the iteration runs behind it
LBFGS_RULE void ls_accept(LbfgsDev* st, double t_acc, double f_acc, double gtd_acc, int slot) {
    LbfgsTick& k = st->tick;
    k.action = LS_ACT_ACCEPT; k.from_idle = 0; k.t_acc = t_acc; k.f_acc = f_acc; k.gtd_acc = gtd_acc; k.acc_slot = slot;
    st->ls.accepted += 1; st->ls.stalled += t_acc == 0.0;
    st->t = t_acc;                                                  // s = t_acc d: the pair of the iteration that follows
}

// One tick (torch's order of tests) on the trial's loss, g.d, sum|g|, max|g| and max|d|: leaves the next trial step, or accept(slot, t,
// loss), or -- a non-finite loss or gradient at a trial -- back to the best point held and frozen (2).
LBFGS_RULE void ls_decide(LbfgsDev* st, const LbfgsCfg& cfg, const LsCfg& lc, double loss, double gtd_new, double g1, double gmax, double dmax) {
    LsDev& ls = st->ls;
    LbfgsTick& k = st->tick;
    (void)gmax;                                                     // (the iteration's freeze rule reads the accepted gradient's)
    if (st->frozen) { k.action = LS_ACT_NONE; return; }
    const int slot = ls.slot_new;
    ls.evals_total += 1;
    if (ls.state == LS_IDLE) {                                      // an evaluation at theta0: the iteration's own rules decide
        k.action = LS_ACT_ACCEPT; k.from_idle = 1; k.t_acc = 0.0; k.f_acc = loss; k.gtd_acc = 0.0; k.acc_slot = slot;
        return;
    }
    if (ls.ls_evals == 0) ls.dnorm = dmax;
    ls.ls_evals += 1;
    if (!(__builtin_isfinite(loss) && __builtin_isfinite(g1))) {    // never leave theta at such a trial
        k.action = LS_ACT_RESTORE; k.from_idle = 0;
        k.t_acc = ls.state == LS_ZOOM ? ls.b[ls.low_pos] : 0.0;
        lbfgs_freeze(st, LBFGS_FROZEN_NONFINITE, true);
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
                k.action = LS_ACT_TRIAL; ls.did = LS_DID_BRACKET;
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
    // the head of torch's zoom loop: its three ends all accept the low end of the bracket
    long long* end = done ? &ls.end_curv : ls.ls_iter >= lc.max_ls ? &ls.end_max_ls
                   : fabs(b[1] - b[0]) * ls.dnorm < cfg.tol_change ? &ls.end_width : nullptr;
    if (end) {
        const int low = ls.low_pos;
        *end += 1;
        ls_accept(st, b[low], bf[low], bgtd[low], bslot[low]);
        return;
    }
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
    k.action = LS_ACT_TRIAL; ls.did = LS_DID_ZOOM;
}

// behind an accepted point's iteration the search along the new direction starts there (skip: the next evaluation is taken at theta0)
LBFGS_RULE void ls_rearm(LbfgsDev* st, double loss, double gtd, double t, int skip) {
    LsDev& ls = st->ls;
    ls.f0 = loss; ls.gtd0 = gtd; ls.t = t;
    ls.b[0] = 0.0; ls.bf[0] = loss; ls.bgtd[0] = gtd; ls.bslot[0] = LS_START_SLOT;
    ls.b[1] = st->tick.t_acc; ls.bf[1] = loss; ls.bgtd[1] = st->tick.gtd_acc; ls.bslot[1] = LS_START_SLOT;
    ls.low_pos = 0; ls.insuf = 0; ls.ls_iter = 0; ls.ls_evals = 0; ls.slot_new = 0;
    ls.state = skip ? LS_IDLE : LS_BRACKET; ls.did = LS_DID_ACCEPTED;
}
