// Self-test of csrc/gpe_dispatch.h alone (no HIP): built by tests/test_dispatch_cpu.py with g++ -fsanitize=address,undefined, once as the
// product compiles it and once with -DGPE_FAST_BUILD, and run as a child process.  Prints one line per check; exit status 1 on a failure.
#include "../gross-pitaevskii-eigenvalue-problem_amd/csrc/gpe_dispatch.h"

#include <cstdio>
#include <set>
#include <utility>
#include <vector>

static int failures = 0;
static void check(bool ok, const char* what, int a = 0, int b = 0) {
    if (!ok) { printf("FAIL %s (%d, %d)\n", what, a, b); ++failures; }
}

// every input from Lo - 2 to Hi + 2: one call, with the clamped value; each_int: every value once, ascending
template <int Lo, int Hi>
static void range() {
    for (int v = Lo - 2; v <= Hi + 2; ++v) {
        int calls = 0, got = -1000;
        pick_int<Lo, Hi>(v, [&](auto c) {
            static_assert(decltype(c)::value >= Lo && decltype(c)::value <= Hi, "picked outside the range");
            ++calls; got = decltype(c)::value;
        });
        check(calls == 1, "pick_int: calls", v, calls);
        check(got == (v < Lo ? Lo : (v > Hi ? Hi : v)), "pick_int: clamped value", v, got);
    }
    std::vector<int> seen;
    each_int<Lo, Hi>([&](auto c) { seen.push_back(decltype(c)::value); });
    check((int)seen.size() == Hi - Lo + 1, "each_int: count", Lo, (int)seen.size());
    for (size_t i = 0; i < seen.size(); ++i) check(seen[i] == Lo + (int)i, "each_int: value", Lo, seen[i]);
    printf("range %d..%d ok\n", Lo, Hi);
}

using Pairs = std::set<std::pair<int, int>>;
template <class L>
static void pairs(const char* name, L list, const Pairs& want) {
    for (int c = -1; c <= 9; ++c)
        for (int e = -1; e <= 5; ++e) {
            int calls = 0, gc = -1, ge = -1;
            const bool hit = pick_ce(list, c, e, [&](auto C, auto E) { ++calls; gc = C; ge = E; });
            const bool in = want.count({c, e}) != 0;
            check(hit == in, name, c, e);
            check(calls == (in ? 1 : 0), "pick_ce: calls", c, e);
            if (in) check(gc == c && ge == e, "pick_ce: pair handed over", gc, ge);
        }
    Pairs seen;
    int n = 0;
    each_ce(list, [&](auto C, auto E) { seen.insert({C, E}); ++n; });
    check(seen == want && n == (int)want.size(), "each_ce: the list", n, (int)want.size());
    printf("%s ok: %d pairs\n", name, n);
}

int main() {
    // the ranges of the launchers: maps of the cooperative kernels, maps of the pipelined / b6 kernels, a flag, f_backward's
    // maps-in-registers (0: none), n_out of a full build
    range<1, 5>(); range<1, 3>(); range<0, 1>(); range<0, 3>(); range<1, 2>();
#ifdef GPE_FAST_BUILD
    const Pairs train{{1, 0}, {4, 1}, {5, 1}}, forward = train;
    const int max_no = 1;
#else
    const Pairs train{{1, 0}, {3, 1}, {4, 1}, {5, 1}}, forward{{1, 0}, {3, 1}, {4, 1}, {5, 1}, {5, 2}, {7, 3}};
    const int max_no = 2;
#endif
    pairs("ce_train", ce_train{}, train);
    pairs("ce_forward", ce_forward{}, forward);
    pairs("ce_h128_forward", ce_h128_forward{}, Pairs{{1, 0}, {3, 1}, {4, 1}, {5, 2}});
    pairs("ce_h128_reverse", ce_h128_reverse{}, Pairs{{1, 0}, {3, 1}, {4, 1}});
    for (int v = -1; v <= 4; ++v) {
        int calls = 0, got = -1;
        pick_n_out(v, [&](auto c) { ++calls; got = c; });
        check(calls == 1 && got == (v < 1 ? 1 : (v > max_no ? max_no : v)), "pick_n_out", v, got);
    }
    int n = 0;
    each_n_out([&](auto) { ++n; });
    check(n == max_no, "each_n_out", n, max_no);
    printf("n_out 1..%d ok\n", max_no);
    // the forms: four / five maps at H = 128 or for real psi; residual blocks at H <= 64, real psi, two or four maps
    static_assert(coop_form(64, 2, 3, false) && !coop_form(64, 2, 4, false) && coop_form(64, 1, 5, false) && coop_form(128, 2, 5, false), "");
    static_assert(coop_form(32, 1, 2, true) && coop_form(64, 1, 4, true) && !coop_form(64, 1, 3, true) && !coop_form(64, 2, 2, true) && !coop_form(128, 1, 2, true), "");
    static_assert(head_form(64, 3, 1) && !head_form(64, 1, 1) && !head_form(64, 4, 2) && !head_form(128, 4, 1), "");
    static_assert(pipe_form(32, 5) && pipe_form(64, 4) && !pipe_form(64, 5) && !pipe_form(128, 1), "");
    printf("%s %d\n", failures ? "failed" : "done", failures);
    return failures ? 1 : 0;
}
