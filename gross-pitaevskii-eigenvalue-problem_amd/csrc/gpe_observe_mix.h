// gpe_observe_mix.h -- observables of a two-component mixture state (gpe_config.mixture) on a point set, formed on the device from the
// full NN output jets O [C][2][ld], C = 1 + 2 D: the mixture instances of the two-pass chain of gpe_observe.h, with a record of their own
// (include/gpe_hip.h: struct gpe_mixture_observables -- norms, energy parts, one chemical potential per component, overlap of the
// densities, moments, peak densities and the residuals of the state normalised to the target norms).  Replaces the host-side sums of
// tools/accuracy_mixture.py:state (the reference has no mixture).
//
// Launch chain (all on the engine's stream, nothing synchronises):
//   k_mixobs_pass1   per point u_a and its derivatives as k_head_mix forms them (fp32: perturb_scale * O), then the 23 summands and the
//                    2 maxima in fp64; one partial row of MO_ROW doubles per workgroup into a slab
//   k_mixobs_reduce  one workgroup adds the slab rows in index order -> raw totals
//   k_mixobs_pass2   with I_a and mu_a from the totals: sum |H_a[v] v_a - mu_a v_a|^2 per component, one partial pair per workgroup
//   k_mixobs_finish  one workgroup adds those partials in index order and writes the struct (staging slot or monitor ring)
// The discipline is the scalar chain's: every point belongs to a fixed thread, every partial to a fixed slab row, every sum is added in
// a fixed tree, no atomics -- a record repeats bit for bit.  The couplings and target norms (MixPhys) travel by value: they are those in
// force at the launch.  WQ as in gpe_observe.h: the bound set's quadrature weights in every sum, the plain maximum.
#pragma once
#include "gpe_observe.h"

// raw sums over the points; a = component (0, 1), k = axis
enum { MO_S = 0,       // [2] sum u_a^2
       MO_K = 2,       // [2] sum |grad u_a|^2
       MO_P = 4,       // [2] sum V u_a^2
       MO_L = 6,       // [2] sum u_a lap u_a
       MO_Q = 8,       // [3] sum u_1^4, sum u_2^4, sum u_1^2 u_2^2
       MO_X = 11,      // [2][3] sum x_k u_a^2
       MO_XX = 17,     // [2][3] sum x_k^2 u_a^2
       MO_NSUM = 23,
       MO_MAX = 23,    // [2] max u_a^2
       MO_COUNT = 25,
       MO_ROW = 32 };  // doubles per slab row

// u-jets of both components of point m in fp32, exactly as k_head_mix forms them
template <int D>
GPE_DEV void mixobs_point(const Phys& ph, const float* __restrict__ x, const float* __restrict__ O, int64_t ld, int64_t m, float* xv,
                          float (&U)[2][1 + 2 * D]) {
    constexpr int C = 1 + 2 * D;
#pragma unroll
    for (int k = 0; k < D; ++k) xv[k] = x[m * D + k];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
#pragma unroll
        for (int c = 0; c < C; ++c) U[o][c] = ph.perturb_scale * O[((int64_t)c * 2 + o) * ld + m];
    }
}

template <int D, bool WQ = false>
__global__ __launch_bounds__(OBS_THREADS) void k_mixobs_pass1(Phys ph, const float* __restrict__ x, const float* __restrict__ Vpre,
                                                              const float* __restrict__ O, int64_t N, int64_t ld, double* __restrict__ slab,
                                                              const float* __restrict__ qw = nullptr) {
    constexpr int C = 1 + 2 * D;
    __shared__ double lds[(OBS_THREADS / 64) * MO_COUNT];
    double acc[MO_COUNT];
#pragma unroll
    for (int k = 0; k < MO_COUNT; ++k) acc[k] = 0.0;
    for (int64_t m = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x; m < N; m += (int64_t)gridDim.x * OBS_THREADS) {
        float xv[3] = {0.f, 0.f, 0.f};
        float U[2][C];
        mixobs_point<D>(ph, x, O, ld, m, xv, U);
        const double V = (double)potential_at(ph, xv, Vpre, m);
        double q = 1.0;
        if constexpr (WQ) q = (double)qw[m];
        double rho[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const double u = (double)U[a][0];
            double g2 = 0.0, lap = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) { const double uk = (double)U[a][1 + k]; g2 += uk * uk; lap += (double)U[a][1 + D + k]; }
            rho[a] = u * u;
            if constexpr (WQ) {
                acc[MO_S + a] += q * rho[a]; acc[MO_K + a] += q * g2; acc[MO_P + a] += q * (V * rho[a]); acc[MO_L + a] += q * (u * lap);
            } else {
                acc[MO_S + a] += rho[a]; acc[MO_K + a] += g2; acc[MO_P + a] += V * rho[a]; acc[MO_L + a] += u * lap;
            }
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double xk = (double)xv[k];
                if constexpr (WQ) { acc[MO_X + 3 * a + k] += q * (xk * rho[a]); acc[MO_XX + 3 * a + k] += q * (xk * xk * rho[a]); }
                else { acc[MO_X + 3 * a + k] += xk * rho[a]; acc[MO_XX + 3 * a + k] += xk * xk * rho[a]; }
            }
            acc[MO_MAX + a] = fmax(acc[MO_MAX + a], rho[a]);      // (fmax drops NaNs: k_mixobs_finish takes the NaN of the norm instead)
        }
        if constexpr (WQ) {
            acc[MO_Q + 0] += q * (rho[0] * rho[0]); acc[MO_Q + 1] += q * (rho[1] * rho[1]); acc[MO_Q + 2] += q * (rho[0] * rho[1]);
        } else {
            acc[MO_Q + 0] += rho[0] * rho[0]; acc[MO_Q + 1] += rho[1] * rho[1]; acc[MO_Q + 2] += rho[0] * rho[1];
        }
    }
    const double r = obs_block_reduce<MO_COUNT>(acc, MO_NSUM, lds);
    if (threadIdx.x < MO_COUNT) slab[(size_t)blockIdx.x * MO_ROW + threadIdx.x] = r;
}

__global__ __launch_bounds__(OBS_THREADS) void k_mixobs_reduce(const double* __restrict__ slab, int rows, double* __restrict__ raw) {
    __shared__ double lds[(OBS_THREADS / 64) * MO_COUNT];
    const double r = obs_slab_total<MO_COUNT, MO_ROW>(slab, rows, MO_NSUM, lds);
    if (threadIdx.x < MO_COUNT) raw[threadIdx.x] = r;
}

// the fields of the normalised state that follow from the raw totals (formulas of include/gpe_hip.h: struct gpe_mixture_observables)
struct MixObsParts { double I[2], kin[2], pot[2], inter[3], mu[2], mu_lap[2]; };
GPE_DEV MixObsParts mixobs_parts(const Phys& ph, const MixPhys& mx, const double* __restrict__ raw, double dv) {
#pragma clang fp contract(off)      // both callers round alike, and no product is fused into a sum of k_mixobs_finish
    MixObsParts q;
    const double c = (double)ph.kin, s[2] = {raw[MO_S], raw[MO_S + 1]}, n[2] = {(double)mx.n[0], (double)mx.n[1]};
    const double q12 = (double)mx.g[2] * raw[MO_Q + 2] / (s[0] * s[1] * dv);          // g_12 Q_12 / (s_1 s_2 dv)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        q.I[a] = dv * s[a];
        q.kin[a] = c * n[a] * raw[MO_K + a] / s[a];
        q.pot[a] = n[a] * raw[MO_P + a] / s[a];
        const double qaa = (double)mx.g[a] * n[a] * raw[MO_Q + a] / (s[a] * s[a] * dv);      // g_aa n_a Q_aa / (s_a^2 dv)
        q.inter[a] = 0.5 * n[a] * qaa;
        const double tail = raw[MO_P + a] / s[a] + qaa + n[1 - a] * q12;
        q.mu[a] = c * raw[MO_K + a] / s[a] + tail;
        q.mu_lap[a] = -c * raw[MO_L + a] / s[a] + tail;
    }
    q.inter[2] = n[0] * n[1] * q12;
    return q;
}

template <int D, bool WQ = false>
__global__ __launch_bounds__(OBS_THREADS) void k_mixobs_pass2(Phys ph, MixPhys mx, const float* __restrict__ x, const float* __restrict__ Vpre,
                                                              const float* __restrict__ O, int64_t N, int64_t ld,
                                                              const double* __restrict__ raw, double dv, double* __restrict__ slab,
                                                              const float* __restrict__ qw = nullptr) {
    constexpr int C = 1 + 2 * D;
    __shared__ double lds[(OBS_THREADS / 64) * 2];
    const MixObsParts p = mixobs_parts(ph, mx, raw, dv);
    // v_a = f_a u_a, f_a^2 = n_a / I_a:  H_a[v] v_a - mu_a v_a = f_a (-c lap u_a + (V - mu_a) u_a + (g_aa f_a^2 u_a^2 + g_12 f_b^2 u_b^2) u_a)
    const double f2[2] = {(double)mx.n[0] / p.I[0], (double)mx.n[1] / p.I[1]}, f[2] = {sqrt(f2[0]), sqrt(f2[1])};
    const double c = (double)ph.kin, g12 = (double)mx.g[2];
    double acc[2] = {0.0, 0.0};
    for (int64_t m = (int64_t)blockIdx.x * OBS_THREADS + threadIdx.x; m < N; m += (int64_t)gridDim.x * OBS_THREADS) {
        float xv[3] = {0.f, 0.f, 0.f};
        float U[2][C];
        mixobs_point<D>(ph, x, O, ld, m, xv, U);
        const double V = (double)potential_at(ph, xv, Vpre, m);
        const double w[2] = {f2[0] * (double)U[0][0] * (double)U[0][0], f2[1] * (double)U[1][0] * (double)U[1][0]};      // v_a^2
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const double u = (double)U[a][0];
            double lap = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) lap += (double)U[a][1 + D + k];
            const double r = f[a] * (-c * lap + (V - p.mu[a]) * u + ((double)mx.g[a] * w[a] + g12 * w[1 - a]) * u);
            if constexpr (WQ) acc[a] += (double)qw[m] * (r * r);
            else acc[a] += r * r;
        }
    }
    const double r = obs_block_reduce<2>(acc, 2, lds);
    if (threadIdx.x < 2) slab[(size_t)blockIdx.x * MO_ROW + threadIdx.x] = r;
}

__global__ __launch_bounds__(OBS_THREADS) void k_mixobs_finish(Phys ph, MixPhys mx, const double* __restrict__ slab, int rows,
                                                               const double* __restrict__ raw, double dv, double n_points,
                                                               const OptDev* __restrict__ od, struct gpe_mixture_observables* __restrict__ dst) {
#pragma clang fp contract(off)      // energy is the sum of the seven fields as stored, to the bit
    __shared__ double lds[(OBS_THREADS / 64) * 2];
    __shared__ double r2[2];
    const double t = obs_slab_total<2, MO_ROW>(slab, rows, 2, lds);
    if (threadIdx.x < 2) r2[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const MixObsParts p = mixobs_parts(ph, mx, raw, dv);
    struct gpe_mixture_observables o;
    o.n = n_points; o.dv = dv; o.step = (double)od->step;
    double e = 0.0;
    for (int a = 0; a < 2; ++a) { o.norm[a] = p.I[a]; o.kin[a] = p.kin[a]; o.pot[a] = p.pot[a]; o.mu[a] = p.mu[a]; o.mu_lap[a] = p.mu_lap[a]; }
    for (int a = 0; a < 2; ++a) e += p.kin[a];
    for (int a = 0; a < 2; ++a) e += p.pot[a];
    for (int k = 0; k < 3; ++k) { o.inter[k] = p.inter[k]; e += p.inter[k]; }
    o.energy = e;
    o.overlap = raw[MO_Q + 2] / sqrt(raw[MO_Q] * raw[MO_Q + 1]);
    for (int a = 0; a < 2; ++a) {
        for (int k = 0; k < 3; ++k) {
            const double mk = raw[MO_X + 3 * a + k] / raw[MO_S + a];
            o.mean_x[a][k] = mk;
            o.var_x[a][k] = raw[MO_XX + 3 * a + k] / raw[MO_S + a] - mk * mk;
        }
        o.peak_density[a] = (double)mx.n[a] * raw[MO_MAX + a] / p.I[a];      // I_a = NaN (a diverged state) makes this NaN too, whatever fmax kept
        o.res_rms[a] = sqrt(dv * r2[a]);
    }
    o.res_rms_total = sqrt(o.res_rms[0] * o.res_rms[0] + o.res_rms[1] * o.res_rms[1]);
    *dst = o;
}
