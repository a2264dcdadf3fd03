// Stand-alone driver of csrc/gpe_lbfgs_rules.h -- the scalar rules of the device-resident L-BFGS: the line search's state machine, its
// re-arm behind an accepted point's iteration, the freeze and the judged-point rule -- for tests/test_lbfgs_rules_cpu.py, which builds it
// with the address and undefined-behaviour sanitizers and runs it as a child process.  No HIP, no GPU, nothing loaded into Python.
//
// argv[1] is a trace of whitespace-separated words; doubles are C hex floats (or nan, inf):
//   run NAME lr tol_grad tol_change stop_loss m c1 c2 max_ls     a reset state (as lbfgs_reset leaves it, the line search's buffers held)
//   tick loss gtd g1 gmax dmax                                   ls_decide on one evaluation; if it ACCEPTS a point the next words are
//   iter CODE loss gtd t skip                                    what the iteration hands back: CODE != 0: it froze (lbfgs_freeze), else
//                                                                ls_rearm with the new direction's g.d, its first step and the skip flag
// One line per tick on stdout, after the iteration if there was one (the fields: see the printf below), then "done TICKS".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include "../gross-pitaevskii-eigenvalue-problem_amd/csrc/gpe_lbfgs_rules.h"

static std::ifstream in;

static std::string word() {
    std::string w;
    if (!(in >> w)) { fprintf(stderr, "trace ends early\n"); exit(2); }
    return w;
}
static long long integer() { return strtoll(word().c_str(), nullptr, 10); }
static double real() { return strtod(word().c_str(), nullptr); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s TRACE\n", argv[0]); return 2; }
    in.open(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::unique_ptr<LbfgsDev> st(new LbfgsDev);          // on the heap at exactly its size: an index past b[1] or rec[15] is a report
    std::unique_ptr<float[]> buf(new float[4]);
    LbfgsCfg cfg = {};
    LsCfg lc = {};
    std::string name, w;
    long long n_ticks = 0, k = 0;
    while (in >> w) {
        if (w == "run") {
            name = word();
            cfg.lr = real(); cfg.tol_grad = real(); cfg.tol_change = real(); cfg.stop_loss = real(); cfg.m = (int)integer();
            lc.kind = 1; lc.c1 = real(); lc.c2 = real(); lc.max_ls = (int)integer();
            memset(st.get(), 0, sizeof(LbfgsDev));
            st->H_diag = 1.0; st->prev_loss = INFINITY;
            st->ls.slots = buf.get(); st->ls.theta0 = buf.get() + 3;
            k = 0;
            continue;
        }
        if (w != "tick" || name.empty()) { fprintf(stderr, "trace: expected 'run' or 'tick', found '%s'\n", w.c_str()); return 2; }
        const double loss = real(), gtd = real(), g1 = real(), gmax = real(), dmax = real();
        ls_decide(st.get(), cfg, lc, loss, gtd, g1, gmax, dmax);
        const LbfgsTick tk = st->tick;                   // the decision, before the iteration behind it
        if (tk.action == LS_ACT_ACCEPT) {
            if (word() != "iter") { fprintf(stderr, "%s tick %lld: the rules accept a point, the trace has no iteration\n", name.c_str(), k); return 3; }
            const int code = (int)integer();
            const double f = real(), gtd_d = real(), t = real();
            const int skip = (int)integer();
            if (code) lbfgs_freeze(st.get(), code, true);
            else ls_rearm(st.get(), f, gtd_d, t, skip);
        }
        const LsDev& ls = st->ls;
        if (ls.slot_new < 0 || ls.slot_new >= LS_SLOTS || ls.slot_new == (ls.state == LS_IDLE ? -1 : ls.bslot[0]) ||
            (ls.state == LS_ZOOM && ls.slot_new == ls.bslot[1])) { fprintf(stderr, "%s tick %lld: slot %d is not free\n", name.c_str(), k, ls.slot_new); return 3; }
        printf("%s %lld action %d did %d state %d t %a slot_new %d b %a %a bf %a %a bgtd %a %a bslot %d %d low_pos %d insuf %d ls_iter %d ls_evals %d "
               "evals_total %lld accepted %lld end_max_ls %lld end_width %lld end_curv %lld stalled %lld frozen %d rec_frozen %a f0 %a gtd0 %a dnorm %a "
               "t_acc %a f_acc %a gtd_acc %a acc_slot %d from_idle %d lb_t %a at_start %d\n",
               name.c_str(), k, tk.action, ls.did, ls.state, ls.t, ls.slot_new, ls.b[0], ls.b[1], ls.bf[0], ls.bf[1], ls.bgtd[0], ls.bgtd[1], ls.bslot[0],
               ls.bslot[1], ls.low_pos, ls.insuf, ls.ls_iter, ls.ls_evals, ls.evals_total, ls.accepted, ls.end_max_ls, ls.end_width, ls.end_curv,
               ls.stalled, st->frozen, st->rec[LBR_FROZEN], ls.f0, ls.gtd0, ls.dnorm, tk.t_acc, tk.f_acc, tk.gtd_acc, tk.acc_slot, tk.from_idle, st->t,
               (int)lbfgs_judged_at_start(st.get()));
        ++k; ++n_ticks;
    }
    printf("done %lld\n", n_ticks);
    return 0;
}
