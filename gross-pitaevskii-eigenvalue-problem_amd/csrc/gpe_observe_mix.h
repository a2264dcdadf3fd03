// gpe_observe_mix.h -- the mixture kind of the observables chain of gpe_observe.h: a two-component state (gpe_config.mixture) on a point
// set, from the full NN output jets O [C][2][ld], C = 1 + 2 D, into a record of its own (include/gpe_hip.h: struct
// gpe_mixture_observables -- norms, energy parts, one chemical potential per component, overlap of the densities, moments, peak densities
// and the residuals of the state normalised to the target norms).  Replaces the host-side sums of tools/accuracy_mixture.py:state (the
// reference has no mixture).
// Pass 1 takes 23 summands and 2 maxima per point, pass 2 one squared residual per component.  The couplings and target norms (MixPhys)
// travel by value: they are those in force at the launch.
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

struct ObsMix {
    enum { COUNT = MO_COUNT, NSUM = MO_NSUM, ROW = MO_ROW, NRES = 2 };
    using Arg = MixPhys;
    using Record = struct gpe_mixture_observables;

    // both components in fp32, exactly as k_head_mix forms them
    template <int D>
    static GPE_DEV void jets(const Phys& ph, float, const float* __restrict__ O, const float* const* __restrict__, int64_t ld, int64_t m,
                             const float*, float (&U)[2][1 + 2 * D]) {
        constexpr int C = 1 + 2 * D;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
#pragma unroll
            for (int c = 0; c < C; ++c) U[o][c] = ph.perturb_scale * O[((int64_t)c * 2 + o) * ld + m];
        }
    }

    template <int D, bool WQ>
    static GPE_DEV void summands(const Phys&, const float* xv, const float (&U)[2][1 + 2 * D], double V, double q, double (&acc)[COUNT]) {
        double rho[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const double u = (double)U[a][0];
            double g2 = 0.0, lap = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) { const double uk = (double)U[a][1 + k]; g2 += uk * uk; lap += (double)U[a][1 + D + k]; }
            rho[a] = u * u;
            acc[MO_S + a] += obs_w<WQ>(q, rho[a]); acc[MO_K + a] += obs_w<WQ>(q, g2); acc[MO_P + a] += obs_w<WQ>(q, V * rho[a]);
            acc[MO_L + a] += obs_w<WQ>(q, u * lap);
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double xk = (double)xv[k];
                acc[MO_X + 3 * a + k] += obs_w<WQ>(q, xk * rho[a]); acc[MO_XX + 3 * a + k] += obs_w<WQ>(q, xk * xk * rho[a]);
            }
            acc[MO_MAX + a] = fmax(acc[MO_MAX + a], rho[a]);      // (fmax drops NaNs: fill takes the NaN of the norm instead)
        }
        acc[MO_Q + 0] += obs_w<WQ>(q, rho[0] * rho[0]); acc[MO_Q + 1] += obs_w<WQ>(q, rho[1] * rho[1]); acc[MO_Q + 2] += obs_w<WQ>(q, rho[0] * rho[1]);
    }

    // the fields of the normalised state that follow from the raw totals (formulas of include/gpe_hip.h: struct gpe_mixture_observables)
    struct Parts { double I[2], kin[2], pot[2], inter[3], mu[2], mu_lap[2]; };
    static GPE_DEV Parts parts(const Phys& ph, const MixPhys& mx, const double* __restrict__ raw, double dv) {
#pragma clang fp contract(off)      // both callers round alike, and no product is fused into a sum of fill
        Parts q;
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

    // v_a = f_a u_a, f_a^2 = n_a / I_a:  H_a[v] v_a - mu_a v_a = f_a (-c lap u_a + (V - mu_a) u_a + (g_aa f_a^2 u_a^2 + g_12 f_b^2 u_b^2) u_a)
    struct ResConsts { double mu[2], f2[2], f[2], c, g12; };
    static GPE_DEV ResConsts residual_consts(const Phys& ph, const MixPhys& mx, const double* __restrict__ raw, double dv) {
        const Parts p = parts(ph, mx, raw, dv);
        const double f2[2] = {(double)mx.n[0] / p.I[0], (double)mx.n[1] / p.I[1]};
        return {{p.mu[0], p.mu[1]}, {f2[0], f2[1]}, {sqrt(f2[0]), sqrt(f2[1])}, (double)ph.kin, (double)mx.g[2]};
    }
    template <int D, bool WQ>
    static GPE_DEV void residual(const Phys&, const MixPhys& mx, const ResConsts& k, const float*, const float (&U)[2][1 + 2 * D], double V,
                                 double q, double (&acc)[NRES]) {
        const double w[2] = {k.f2[0] * (double)U[0][0] * (double)U[0][0], k.f2[1] * (double)U[1][0] * (double)U[1][0]};      // v_a^2
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const double u = (double)U[a][0];
            double lap = 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j) lap += (double)U[a][1 + D + j];
            const double r = k.f[a] * (-k.c * lap + (V - k.mu[a]) * u + ((double)mx.g[a] * w[a] + k.g12 * w[1 - a]) * u);
            acc[a] += obs_w<WQ>(q, r * r);
        }
    }

    static GPE_DEV void fill(const Phys& ph, const MixPhys& mx, const double* __restrict__ raw, double dv, const double (&r2)[NRES], Record& o) {
#pragma clang fp contract(off)      // energy is the sum of the seven fields as stored, to the bit
        const Parts p = parts(ph, mx, raw, dv);
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
    }
};
