// gpe_dispatch.h -- runtime values to template arguments, in one place.  Host only: no HIP, plain C++17 (tests/dispatch_selftest.cpp
// includes this header alone).  The launchers of gpe_engine.hip and raise_lds_limits both go through it, so a template range is
// stated once: pick_* hands ONE value of a closed set to a generic lambda as a std::integral_constant (the lambda guards arms with
// `if constexpr`), each_* hands it EVERY value of the same set.
#pragma once
#include <type_traits>

template <int V> using int_c = std::integral_constant<int, V>;

// f(int_c<v>) with v clamped to [Lo, Hi]; f is called exactly once.  A bool is pick_int<0, 1>.
template <int Lo, int Hi, class F>
inline void pick_int(int v, F&& f) {
    static_assert(Lo <= Hi, "empty range");
    if constexpr (Lo == Hi) f(int_c<Lo>{});
    else if (v <= Lo) f(int_c<Lo>{});
    else pick_int<Lo + 1, Hi>(v, f);
}
template <int Lo, int Hi, class F>
inline void each_int(F&& f) {
    f(int_c<Lo>{});
    if constexpr (Lo < Hi) each_int<Lo + 1, Hi>(f);
}

// output components the fused kernels are compiled for: 1 (real psi) and 2 (complex psi, mixtures); kernel-tuning builds 1 alone
#ifdef GPE_FAST_BUILD
#define GPE_MAX_NO 1
#else
#define GPE_MAX_NO 2
#endif
template <class F> inline void pick_n_out(int n_out, F&& f) { pick_int<1, GPE_MAX_NO>(n_out, f); }
template <class F> inline void each_n_out(F&& f) { each_int<1, GPE_MAX_NO>(f); }

// (C, E) = (jet channels, first-derivative channels) pairs that exist: value only (1,0); 1D (3,1); Laplacian-channel training batches
// 2D (4,1), 3D (5,1); full diagonal second derivatives for gpe_forward_jets 2D (5,2), 3D (7,3) -- forward kernels only.  Kernel-tuning
// builds keep (1,0), (4,1), (5,1).  H = 128 (1D / 2D only): the forward kernels take (1,0), (3,1), (4,1), (5,2), the reverse (1,0), (3,1), (4,1).
template <int C, int E> struct ce {};
template <class... P> struct ce_list {};
#ifdef GPE_FAST_BUILD
using ce_train = ce_list<ce<1, 0>, ce<4, 1>, ce<5, 1>>;
using ce_forward = ce_train;
#else
using ce_train = ce_list<ce<1, 0>, ce<3, 1>, ce<4, 1>, ce<5, 1>>;
using ce_forward = ce_list<ce<1, 0>, ce<3, 1>, ce<4, 1>, ce<5, 1>, ce<5, 2>, ce<7, 3>>;
#endif
using ce_h128_forward = ce_list<ce<1, 0>, ce<3, 1>, ce<4, 1>, ce<5, 2>>;
using ce_h128_reverse = ce_list<ce<1, 0>, ce<3, 1>, ce<4, 1>>;

template <int... C, int... E, class F>
inline void each_ce(ce_list<ce<C, E>...>, F&& f) { (f(int_c<C>{}, int_c<E>{}), ...); }
// f(int_c<C>, int_c<E>) if the list holds (c, e); returns whether it does (the caller reports a pair that does not exist)
template <class L, class F>
inline bool pick_ce(L list, int c, int e, F&& f) {
    bool hit = false;
    each_ce(list, [&](auto C, auto E) { if (C == c && E == e) { f(C, E); hit = true; } });
    return hit;
}

// ---- which instances of the fused kernels exist (H = 32 / 64 / 128; NH = hidden -> hidden maps) ----------------------------------------
//   f_forward_coop  <H,C,E,NO,NH,HEAD,RES>   NH 1..5     coop_form; HEAD: head_form; at H = 128 for C <= 4
//   f_backward_coop <H,C,E,NO,NH,B6,RES>     NH 1..5     coop_form; B6: H <= 64, NH 1..3, no RES
//   f_backward_pipe <H,C,E,NO,NH,SEEDS>      NH 1..3     pipe_form; SEEDS: head_form
//   f_forward       <H,C,E,NO,WL,HEAD>       WL 0..1     WL: picked at H <= 64 only; HEAD: head_form
//   f_forward_b6    <H,C,E,NO,WL>            WL 0..1     H <= 64
//   f_backward      <H,C,E,NO,WL,NH>         NH 0..3     <false, 0> at every H; <true, 1..3> (weight gradient in registers) at H <= 64
// NO from pick_n_out, (C, E) from ce_train / ce_forward (H = 128: ce_h128_*).  A runtime value outside a range runs the range's nearer end.
// four / five maps: H = 128, or real psi; residual blocks (RES): H <= 64, real psi, one or two blocks = two or four maps
constexpr bool coop_form(int H, int NO, int NH, bool RES) {
    return (NH <= 3 || H == 128 || NO == 1) && (!RES || (H <= 64 && NO == 1 && (NH == 2 || NH == 4)));
}
// the head in a forward kernel / the seeds in the pipelined reverse kernel: H <= 64, real psi, a batch with derivative channels
constexpr bool head_form(int H, int C, int NO) { return H <= 64 && NO == 1 && C >= 3; }
// pipelined reverse kernel: H <= 64, except H = 64 in 3D (two workgroups' exchange buffers exceed the LDS)
constexpr bool pipe_form(int H, int C) { return H <= 64 && !(H == 64 && C == 5); }
