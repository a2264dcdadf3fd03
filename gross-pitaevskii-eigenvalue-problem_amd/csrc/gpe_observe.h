// gpe_observe.h -- observables of the NORMALISED state on a point set, formed on the device from the full NN output jets
// O [C][n_out][ld], C = 1 + 2 D (value, D first derivatives, D diagonal second derivatives; point index contiguous).  One launch chain,
// instantiated for two KINDS of engine: ObsScalar (below; include/gpe_hip.h: struct gpe_observables -- norm, energy parts, chemical
// potential, <L_z>, density moments, peak density and the residual of the normalised state) and ObsMix (gpe_observe_mix.h: struct
// gpe_mixture_observables).  Replaces the host-side sums of tools/accuracy_cfg4.py:state_numbers (the reference has no counterpart: it
// never evaluates the energy of a trained state).
//
// Launch chain (all on the engine's stream, nothing synchronises):
//   k_obs_pass1   per point u and its derivatives as the head forms them (fp32), then the kind's summands in fp64;
//                 one partial row per workgroup into a slab
//   k_obs_reduce  one workgroup adds the slab rows in index order -> raw totals
//   k_obs_pass2   with the norms and mu from the totals: the squared residual of the normalised state, one partial (per component) per
//                 workgroup
//   k_obs_finish  one workgroup adds those partials in index order and writes the struct (staging slot or monitor ring)
// Every point belongs to a fixed thread, every partial to a fixed slab row, every sum is added in a fixed tree: no atomics, so a
// record repeats bit for bit (README, "Reproducibility").
// A kind is a type of static members and says only what differs:
//   COUNT, NSUM, ROW, NRES   accumulators per thread (the first NSUM are added, the rest take the maximum), doubles per slab row,
//                            residual sums
//   Arg                      what travels by value besides Phys (in force at the launch)
//   Record                   the struct filled
//   jets<D>                  the u-jets of a point
//   summands<D, WQ>          pass 1: the point's terms into the accumulators
//   parts                    the fields that follow from the raw totals
//   residual_consts, residual<D, WQ>    pass 2: what the totals fix for every point, and the point's squared residual per component
//   fill                     the record from the totals, the parts and the residual sums
// WQ (gpe_observables on the bound set while gpe_bind_weights is in force): every point's summands take its quadrature weight qw[m] --
// the sums approximate integrals with dv * q_i as the measure -- and the peak density stays the plain maximum.  An explicit point set
// and the monitor run the WQ = false instances, which neither read qw nor multiply (obs_w).
#pragma once
#include "gpe_head.h"

#define OBS_THREADS 256
#define OBS_MAX_WG 1024          // slab rows: the grid never exceeds it, whatever the device

template <bool WQ>
GPE_DEV double obs_w(double q, double v) {
    if constexpr (WQ) return q * v;
    else return v;
}

// K values per thread -> per workgroup, in thread k < K of the workgroup (values [0, nsum) are added, the rest take the maximum).
// Wave: shuffle tree over 64 lanes; workgroup: one LDS row per wave, added in wave order.
template <int K>
GPE_DEV double obs_block_reduce(double (&v)[K], int nsum, double* lds /*[waves][K]*/) {
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double q = __shfl_down(t, o, 64);
            t = k < nsum ? t + q : fmax(t, q);
        }
        if ((threadIdx.x & 63) == 0) lds[w * K + k] = t;
    }
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        r = lds[k];
        for (int i = 1; i < nw; ++i) r = k < nsum ? r + lds[i * K + k] : fmax(r, lds[i * K + k]);
    }
    return r;
}

// rows of a slab added in index order by ONE workgroup: thread t takes rows t, t + 256, ..., then the workgroup tree
template <int K, int ROW>
GPE_DEV double obs_slab_total(const double* __restrict__ slab, int rows, int nsum, double* lds) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int r = threadIdx.x; r < rows; r += OBS_THREADS) {
#pragma unroll
        for (int k = 0; k < K; ++k) { const double q = slab[(size_t)r * ROW + k]; v[k] = k < nsum ? v[k] + q : fmax(v[k], q); }
    }
    return obs_block_reduce<K>(v, nsum, lds);
}

template <int D>
GPE_DEV void obs_load_x(const float* __restrict__ x, int64_t m, float* xv) {
#pragma unroll
    for (int k = 0; k < D; ++k) xv[k] = x[m * D + k];
}

// ---- the chain ----------------------------------------------------------------------------------------------------------------------------
// base_norm, bptr: the base function of a scalar engine (a mixture has none)
template <class K, int D, bool WQ = false>
__global__ __launch_bounds__(OBS_THREADS) void k_obs_pass1(Phys ph, float base_norm, const float* __restrict__ x,
                                                           const float* __restrict__ Vpre, const float* __restrict__ O,
                                                           const float* const* __restrict__ bptr, int64_t N, int64_t ld,
                                                           double* __restrict__ slab, const float* __restrict__ qw = nullptr) {
    constexpr int C = 1 + 2 * D;
    __shared__ double lds[(OBS_THREADS / 64) * K::COUNT];
    double acc[K::COUNT];
#pragma unroll
    for (int k = 0; k < K::COUNT; ++k) acc[k] = 0.0;
    for (int64_t m = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x; m < N; m += (int64_t)gridDim.x * OBS_THREADS) {
        float xv[3] = {0.f, 0.f, 0.f};
        float U[2][C];
        obs_load_x<D>(x, m, xv);
        K::template jets<D>(ph, base_norm, O, bptr, ld, m, xv, U);
        const double V = (double)potential_at(ph, xv, Vpre, m);
        double q = 1.0;
        if constexpr (WQ) q = (double)qw[m];
        K::template summands<D, WQ>(ph, xv, U, V, q, acc);
    }
    const double r = obs_block_reduce<K::COUNT>(acc, K::NSUM, lds);
    if (threadIdx.x < K::COUNT) slab[(size_t)blockIdx.x * K::ROW + threadIdx.x] = r;
}

template <class K>
__global__ __launch_bounds__(OBS_THREADS) void k_obs_reduce(const double* __restrict__ slab, int rows, double* __restrict__ raw) {
    __shared__ double lds[(OBS_THREADS / 64) * K::COUNT];
    const double r = obs_slab_total<K::COUNT, K::ROW>(slab, rows, K::NSUM, lds);
    if (threadIdx.x < K::COUNT) raw[threadIdx.x] = r;
}

template <class K, int D, bool WQ = false>
__global__ __launch_bounds__(OBS_THREADS) void k_obs_pass2(Phys ph, typename K::Arg ka, float base_norm, const float* __restrict__ x,
                                                           const float* __restrict__ Vpre, const float* __restrict__ O,
                                                           const float* const* __restrict__ bptr, int64_t N, int64_t ld,
                                                           const double* __restrict__ raw, double dv, double* __restrict__ slab,
                                                           const float* __restrict__ qw = nullptr) {
    constexpr int C = 1 + 2 * D;
    __shared__ double lds[(OBS_THREADS / 64) * K::NRES];
    const auto rc = K::residual_consts(ph, ka, raw, dv);
    double acc[K::NRES];
#pragma unroll
    for (int k = 0; k < K::NRES; ++k) acc[k] = 0.0;
    for (int64_t m = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x; m < N; m += (int64_t)gridDim.x * OBS_THREADS) {
        float xv[3] = {0.f, 0.f, 0.f};
        float U[2][C];
        obs_load_x<D>(x, m, xv);
        K::template jets<D>(ph, base_norm, O, bptr, ld, m, xv, U);
        const double V = (double)potential_at(ph, xv, Vpre, m);
        double q = 1.0;
        if constexpr (WQ) q = (double)qw[m];
        K::template residual<D, WQ>(ph, ka, rc, xv, U, V, q, acc);
    }
    const double r = obs_block_reduce<K::NRES>(acc, K::NRES, lds);
    if (threadIdx.x < K::NRES) slab[(size_t)blockIdx.x * K::ROW + threadIdx.x] = r;
}

template <class K>
__global__ __launch_bounds__(OBS_THREADS) void k_obs_finish(Phys ph, typename K::Arg ka, const double* __restrict__ slab, int rows,
                                                            const double* __restrict__ raw, double dv, double n_points,
                                                            const OptDev* __restrict__ od, typename K::Record* __restrict__ dst) {
    __shared__ double lds[(OBS_THREADS / 64) * K::NRES];
    double r2[K::NRES];
    r2[0] = obs_slab_total<K::NRES, K::ROW>(slab, rows, K::NRES, lds);      // total k in thread k
    if constexpr (K::NRES > 1) {                                            // ... all of them to thread 0
        __shared__ double all[K::NRES];
        if (threadIdx.x < K::NRES) all[threadIdx.x] = r2[0];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K::NRES; ++k) r2[k] = all[k];
    }
    if (threadIdx.x != 0) return;
    typename K::Record o;
    o.n = n_points; o.dv = dv; o.step = (double)od->step;
    K::fill(ph, ka, raw, dv, r2, o);
    *dst = o;
}

// ---- the scalar kind: one real or complex psi ---------------------------------------------------------------------------------------------
// raw sums over the points: rho = |u|^2
enum { OB_I = 0,      // sum rho
       OB_K = 1,      // sum |grad u|^2
       OB_P = 2,      // sum V rho
       OB_S = 3,      // sum Re(u* N(u)), N the engine's nonlinear term (gamma included)
       OB_L = 4,      // sum psi_r D psi_i - psi_i D psi_r, D = x d_y - y d_x   (k_head_pde: rzl)
       OB_LAP = 5,    // sum Re(u* lap u)
       OB_X = 6,      // [3] sum x_k rho
       OB_XX = 9,     // [3] sum x_k^2 rho
       OB_NSUM = 12,
       OB_MAX = 12,   // max rho
       OB_COUNT = 13,
       OB_ROW = 16 }; // doubles per slab row

GPE_DEV int obs_power(const Phys& ph) { return ph.complex_psi ? 3 : ph.p; }      // complex psi: gamma |psi|^2 psi

struct ObsNoArg {};
struct ObsScalar {
    enum { COUNT = OB_COUNT, NSUM = OB_NSUM, ROW = OB_ROW, NRES = 1 };
    using Arg = ObsNoArg;
    using Record = struct gpe_observables;

    // both components in fp32, exactly as k_head_pde forms them
    template <int D>
    static GPE_DEV void jets(const Phys& ph, float base_norm, const float* __restrict__ O, const float* const* __restrict__ bptr, int64_t ld,
                             int64_t m, const float* xv, float (&U)[2][1 + 2 * D]) {
        constexpr int C = 1 + 2 * D;
#pragma unroll
        for (int c = 0; c < C; ++c) U[1][c] = 0.f;
        for (int o = 0; o < ph.n_out; ++o) load_u_jets<C, D>(ph, O, ld, m, o, xv, base_norm, bptr, U[o]);
    }

    template <int D, bool WQ>
    static GPE_DEV void summands(const Phys& ph, const float* xv, const float (&U)[2][1 + 2 * D], double V, double q, double (&acc)[COUNT]) {
        double rho = 0.0, g2 = 0.0, ulap = 0.0;
        for (int o = 0; o < ph.n_out; ++o) {
            const double u = (double)U[o][0];
            rho += u * u;
            double lap = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) { const double uk = (double)U[o][1 + k]; g2 += uk * uk; lap += (double)U[o][1 + D + k]; }
            ulap += u * lap;
        }
        double s, lz = 0.0;
        if (!ph.complex_psi) {
            const double u = (double)U[0][0], a = ph.abs_power ? fabs(u) : u;
            double pw = 1.0;
            for (int i = 0; i < ph.p - 1; ++i) pw *= a;
            s = (double)ph.gamma * pw * u * u;                // u * gamma u^p  |  u * gamma |u|^(p-1) u
        } else {
            s = (double)ph.gamma * rho * rho;
            if constexpr (D >= 2) {
                const double xx = (double)xv[0], yy = (double)xv[1];
                const double Dr = xx * (double)U[0][2] - yy * (double)U[0][1];
                const double Di = xx * (double)U[1][2] - yy * (double)U[1][1];
                lz = (double)U[0][0] * Di - (double)U[1][0] * Dr;
            }
        }
        acc[OB_L] += obs_w<WQ>(q, lz);
        acc[OB_I] += obs_w<WQ>(q, rho); acc[OB_K] += obs_w<WQ>(q, g2); acc[OB_P] += obs_w<WQ>(q, V * rho); acc[OB_S] += obs_w<WQ>(q, s);
        acc[OB_LAP] += obs_w<WQ>(q, ulap);
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double xk = (double)xv[k];
            acc[OB_X + k] += obs_w<WQ>(q, xk * rho); acc[OB_XX + k] += obs_w<WQ>(q, xk * xk * rho);
        }
        acc[OB_MAX] = fmax(acc[OB_MAX], rho);              // (fmax drops NaNs: fill takes the NaN of the norm instead)
    }

    // energy parts of the normalised state from the raw totals (formulas of GPE_RIESZ_VARIATIONAL, include/gpe_hip.h)
    struct Parts { double I, kin, pot, inter, rot, lz, mu, mu_lap; };
    static GPE_DEV Parts parts(const Phys& ph, const double* __restrict__ raw, double dv) {
        Parts q;
        const int p = obs_power(ph);
        const double c = (double)ph.kin, sr = raw[OB_I];
        q.I = dv * sr;
        q.kin = c * raw[OB_K] / sr;
        q.pot = raw[OB_P] / sr;
        q.inter = 2.0 / (double)(p + 1) * (dv * raw[OB_S]) / pow(q.I, 0.5 * (double)(p + 1));
        q.lz = raw[OB_L] / sr;
        q.rot = -(double)ph.omega_rot * q.lz;
        const double tail = q.pot + 0.5 * (double)(p + 1) * q.inter + q.rot;
        q.mu = q.kin + tail;
        q.mu_lap = -c * raw[OB_LAP] / sr + tail;
        return q;
    }

    struct ResConsts { double mu, is1, isp, c, g, Om; };
    static GPE_DEV ResConsts residual_consts(const Phys& ph, const Arg&, const double* __restrict__ raw, double dv) {
        const Parts q = parts(ph, raw, dv);
        const int p = obs_power(ph);
        return {q.mu, 1.0 / sqrt(q.I), pow(q.I, -0.5 * (double)p), (double)ph.kin, (double)ph.gamma, (double)ph.omega_rot};
    }
    // |H[phi] phi - mu phi|^2, phi = u / sqrt(I)
    template <int D, bool WQ>
    static GPE_DEV void residual(const Phys& ph, const Arg&, const ResConsts& k, const float* xv, const float (&U)[2][1 + 2 * D], double V,
                                 double q, double (&acc)[NRES]) {
        double lin[2] = {0.0, 0.0}, non[2] = {0.0, 0.0};          // linear part of H u, nonlinear term N(u)
        for (int o = 0; o < ph.n_out; ++o) {
            double lap = 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j) lap += (double)U[o][1 + D + j];
            lin[o] = -k.c * lap + V * (double)U[o][0];
        }
        if (!ph.complex_psi) {
            const double u = (double)U[0][0], a = ph.abs_power ? fabs(u) : u;
            double pw = 1.0;
            for (int i = 0; i < ph.p - 1; ++i) pw *= a;
            non[0] = k.g * pw * u;
        } else {
            const double ur = (double)U[0][0], ui = (double)U[1][0], rho = ur * ur + ui * ui;
            non[0] = k.g * rho * ur; non[1] = k.g * rho * ui;
            if constexpr (D >= 2) {                               // -Omega L_z psi = i Omega (x d_y - y d_x) psi
                const double xx = (double)xv[0], yy = (double)xv[1];
                const double Dr = xx * (double)U[0][2] - yy * (double)U[0][1];
                const double Di = xx * (double)U[1][2] - yy * (double)U[1][1];
                lin[0] += -k.Om * Di; lin[1] += k.Om * Dr;
            }
        }
        for (int o = 0; o < ph.n_out; ++o) {
            const double r = (lin[o] - k.mu * (double)U[o][0]) * k.is1 + non[o] * k.isp;
            acc[0] += obs_w<WQ>(q, r * r);
        }
    }

    static GPE_DEV void fill(const Phys& ph, const Arg&, const double* __restrict__ raw, double dv, const double (&r2)[NRES], Record& o) {
        const Parts q = parts(ph, raw, dv);
        o.norm = q.I;
        o.kin = q.kin; o.pot = q.pot; o.inter = q.inter; o.rot = q.rot;
        o.energy = q.kin + q.pot + q.inter + q.rot;
        o.mu = q.mu; o.mu_lap = q.mu_lap; o.lz = q.lz;
        for (int k = 0; k < 3; ++k) {
            const double mk = raw[OB_X + k] / raw[OB_I];
            o.mean_x[k] = mk;
            o.var_x[k] = raw[OB_XX + k] / raw[OB_I] - mk * mk;
        }
        o.peak_density = raw[OB_MAX] / q.I;              // I = NaN (a diverged state) makes this NaN too, whatever fmax kept
        o.res_rms = sqrt(dv * r2[0]);
    }
};

// ---- keeper (gpe_bind_keeper, gpe_mixture_keeper): the best parameters by one field of the monitor's records, kept on the device ------------
// The record is struct gpe_observables or struct gpe_mixture_observables: all doubles, at most KEEP_REC_MAX of them, so the keeper
// handles it as rec_doubles doubles, one per lane of its wave.
// Two launches directly behind k_obs_finish on the engine's stream, never captured:
//   k_keep_decide  one wave reads the ring slot just written, applies the rule (gpe_pinn/keeper.py restates it), files the record and
//                  the counters, raises or clears the copy flag, and fires the optimiser's own stop (od->stopped) when patience runs out
//   k_keep_copy    theta -> theta_best where the flag is raised.  A launch of its own: the stream orders it behind the decision, so no
//                  workgroup can see a half-written flag; its grid is a function of P alone
#define KEEP_REC_MAX 64
struct KeepDev {
    double best;                  // metric of the kept record (+inf: nothing kept)
    double rec[KEEP_REC_MAX];     // the kept record (its first rec_doubles doubles)
    long long seen, kept, since_best;      // records judged / records kept / records since the last one kept
    int copy;                     // this record improves: k_keep_copy copies
    int stopped;                  // the keeper's patience fired the stop
};
static_assert(sizeof(struct gpe_observables) <= KEEP_REC_MAX * sizeof(double) && sizeof(struct gpe_mixture_observables) <= KEEP_REC_MAX * sizeof(double),
              "the keeper files one double of the record per lane");
#define KEEP_THREADS 256
#define KEEP_MAX_WG 256

// field: index of the chosen double in the record.  Lower is better; a non-finite candidate is no improvement.
__global__ __launch_bounds__(64) void k_keep_decide(const double* __restrict__ src, int field, int rec_doubles, double min_delta,
                                                    long long patience, KeepDev* __restrict__ kd, OptDev* __restrict__ od) {
    const int t = threadIdx.x;
    // every lane reads what the rule needs before any lane writes
    const double m = src[field], best = kd->best;
    const double mine = t < rec_doubles ? src[t] : 0.0;
    const long long since = kd->since_best;
    const bool better = isfinite(m) && m < best - min_delta;
    if (better && t < rec_doubles) kd->rec[t] = mine;                        // the record, one double per lane
    if (t != 0) return;
    const long long since_new = better ? 0 : since + 1;
    if (better) { kd->best = m; kd->kept += 1; }
    kd->copy = better ? 1 : 0;
    kd->since_best = since_new;
    kd->seen += 1;
    if (patience > 0 && since_new >= patience && !od->stopped) {             // the fields the loss-based early stop uses (k_update)
        od->stopped = 1; od->stop_step = od->step;
        kd->stopped = 1;
    }
}

// P floats, 16 bytes per access where both pointers allow it, the last P % 4 (or all of them) one by one
__global__ __launch_bounds__(KEEP_THREADS) void k_keep_copy(const KeepDev* __restrict__ kd, const float* __restrict__ theta,
                                                            float* __restrict__ theta_best, int P) {
    if (!kd->copy) return;
    const bool wide = ((((uintptr_t)theta) | ((uintptr_t)theta_best)) & 15) == 0;
    const int n4 = wide ? P / 4 : 0;
    const float4* s4 = (const float4*)theta;
    float4* d4 = (float4*)theta_best;
    for (int i = blockIdx.x * KEEP_THREADS + threadIdx.x; i < n4; i += gridDim.x * KEEP_THREADS) d4[i] = s4[i];
    for (int i = 4 * n4 + blockIdx.x * KEEP_THREADS + threadIdx.x; i < P; i += gridDim.x * KEEP_THREADS) theta_best[i] = theta[i];
}
