/*
 * gpe_hip.h -- C ABI of libgpe_hip.so: the MI355X (gfx950) engine for the Gross-Pitaevskii
 * eigenvalue-residual PINN training step.
 *
 * The reference (LevBahn/Gross-Pitaevskii-Eigenvalue-problem) has no FFI for this path: it is a set of
 * Python methods on torch tensors.  Each entry point below names the reference code it replaces
 * (paths relative to /root/reference; "refine/" = Gross-Pitaevskii/src/final/refine/,
 * "nb cN:Lm" = Gross_Pitaevskii_1D_power_Test.ipynb code cell N, line m).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  d_* pointers are DEVICE pointers
 *     (e.g. tensor.data_ptr() of a PyTorch-ROCm tensor used as storage); h_* are host pointers.
 *   - Every function returns GPE_OK (0) or a negative gpe_status; gpe_last_error() gives the text.
 *     No exception crosses the ABI.
 *   - A handle is single-device and not thread-safe.  One process per GPU.  Data-parallel exchange: either
 *     by the engine itself -- gpe_comm_unique_id / gpe_comm_init create an RCCL communicator and gpe_step_dp /
 *     gpe_run_dp issue both all-reduces of a step on a dedicated stream -- or by the caller, on the two device
 *     buffers exposed by gpe_exchange_sums() / gpe_exchange_grad() between the three phases of a step.
 *   - All kernels run on the stream given at gpe_create() (NULL = the legacy default stream).
 *   - Parameters are one flat fp32 vector in torch state_dict order:
 *       network.0.weight [out,in] row-major, network.0.bias, network.2.weight, ...
 *     (refine/harmonic_pinn_simulation.py:84-93).
 *   - Derivative "jets": channel 0 = value, 1..d = d/dx_k, d+1..2d = d2/dx_k^2 (C = 1+2d channels).
 */
#ifndef GPE_HIP_H
#define GPE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_ABI_VERSION 2
#define GPE_MAX_LAYERS 12 /* entries of layers[]: [d, H_1, ..., H_L, out] */
#define GPE_MAX_ORTH 4
#define GPE_MAX_DIM 3

typedef enum gpe_status {
    GPE_OK = 0,
    GPE_ERR_INVALID = -1,     /* bad argument / unsupported configuration (ValueError in the reference: refine/harmonic_pinn_simulation.py:143) */
    GPE_ERR_HIP = -2,         /* HIP runtime error */
    GPE_ERR_NONFINITE = -3,   /* loss or gradient not finite; parameters were NOT updated */
    GPE_ERR_STATE = -4,       /* call sequence error (e.g. step before bind_points) */
    GPE_ERR_NOMEM = -5
} gpe_status;

enum { GPE_ACT_TANH = 0, GPE_ACT_TANH_PLUS1 = 1 };                         /* nb c6:L38 ; refine/harmonic_pinn_simulation.py:41-49 */
enum { GPE_POT_HARMONIC = 0, GPE_POT_GAUSSIAN = 1, GPE_POT_PERIODIC = 2,   /* nb c6:L63-79 ; refine/...:136-144 */
       GPE_POT_PRECOMPUTED = 3, GPE_POT_NONE = 4 };
enum { GPE_SCHED_CONST = 0, GPE_SCHED_COSINE_LOSS = 1, GPE_SCHED_PLATEAU = 2 }; /* refine/...:312-314,361 (quirk Q4) ; nb c10:L76-78,L103 */
enum { GPE_PATH_AUTO = 0, GPE_PATH_GENERIC = 1, GPE_PATH_FUSED = 2 };
/* analytic base phi_n of the perturbation ansatz u = phi_n + s*NN: Hermite (refine/harmonic_pinn_simulation.py:95-119),
 * box sine sqrt(2/L) sin((n+1) pi x / L) (refine/box_pinn_simulation.py:99-117), or three caller-supplied arrays
 * (phi, phi', phi'' on the bound points: e.g. the Airy base of refine/gravity_well_pinn_simulation.py:97-173) */
enum { GPE_BASE_HERMITE = 0, GPE_BASE_BOX = 1, GPE_BASE_PRECOMPUTED = 2 };
/* hard boundary factor multiplying the network output in model.forward: none, or sin(pi x / env_L)
 * (refine/box_pinn_simulation.py:119-130) */
enum { GPE_ENV_NONE = 0, GPE_ENV_SIN = 1 };
enum { GPE_RIESZ_PAPER = 0, GPE_RIESZ_SUM = 1, GPE_RIESZ_VARIATIONAL = 2 };
enum { GPE_NET_MLP = 0, GPE_NET_RESIDUAL = 1 };
/* eigenvalue estimate inside the residual:  RAYLEIGH  lambda = sum u (H u) / sum u^2  (refine/harmonic_pinn_simulation.py:186-188; its
 * branch of the gradient vanishes identically);  ENERGY  lambda = [c sum |grad u|^2 + sum V u^2 + gamma sum |u|^(p+1)] / sum u^2,
 * the energy-functional form of the 2D classes (src/gross_pitaevskii_2D.py:192, src/gross_pitaevskii_2D_minimal.py:179; per-point
 * reading of quirk Q1), whose branch of the gradient does NOT vanish and is carried through the reverse pass */
enum { GPE_LAMBDA_RAYLEIGH = 0, GPE_LAMBDA_ENERGY = 1 };

typedef struct gpe_engine gpe_engine; /* opaque */

/* Problem + optimiser description.  Mirrors the literals of refine/harmonic_pinn_simulation.py:963-1009 and
 * nb c20/c22, and the constructor arguments of GrossPitaevskiiPINN (refine/...:57 ; nb c6:L6). */
typedef struct gpe_config {
    int32_t abi_version;          /* = GPE_ABI_VERSION */
    int32_t n_layers;             /* entries used in layers[] */
    int32_t layers[GPE_MAX_LAYERS];
    int32_t activation;           /* GPE_ACT_* */
    int32_t complex_psi;          /* 1: layers[last]==2, psi = out0 + i*out1 */
    float kinetic_coeff;          /* c in -c*laplacian: 1 (refine/...:181) or 0.5 (nb c6:L113) */
    int32_t potential;            /* GPE_POT_* */
    float pot_scale;              /* harmonic: V = pot_scale * sum_k (omega[k]*(x_k - c_k))^2, c = (pot_a, 0, 0): the beta-scaled shifted trap
                                   * V = beta/2 omega^2 (x - center)^2 of refine/vary_potential_parameter_harmonic.py:231-240 is
                                   * pot_scale = beta/2, omega[0] = omega, pot_a = center */
    float omega[GPE_MAX_DIM];
    float pot_a, pot_v0, pot_k;   /* gaussian centre (and harmonic trap centre along x); periodic depth, wave number */
    float omega_rot;              /* rotation frequency Omega: -Omega*L_z psi (complex psi, dim>=2) */
    float gamma;                  /* interaction strength (refine/...:184) */
    int32_t p;                    /* nonlinearity power: gamma*u^p */
    int32_t abs_power;            /* 1: gamma*|u|^(p-1)*u */
    int32_t base_mode;            /* -1 none; n>=0: u = phi_n(x) + perturbation (refine/...:127-134) */
    int32_t base_deriv;           /* 0 exact base derivatives; 1 notebook quirk Q8 (H_n constant, nb c6:L45-47) */
    float perturb_scale;          /* q/normal_const (refine/...:333-340); 1 for the notebook surface */
    float bc_nn_scale;            /* NN scale inside boundary_loss (quirk Q7: 1.0, refine/...:202-206) */
    float w_pde, w_bc, w_norm, w_sym, w_orth;   /* refine/...:347,355 ; nb c10:L97 */
    float sym_sign;               /* +1 even mode, -1 odd mode (nb c6:L150-153) */
    float dx;                     /* quadrature weight of normalization_loss (refine/...:212-217) */
    int64_t n_global;             /* N of the means, over ALL ranks (0: use the bound local count) */
    /* optimiser: torch.optim.Adam defaults + clip_grad_norm_ (refine/...:309,359-360) */
    float lr, beta1, beta2, eps, clip_norm;   /* clip_norm <= 0: no clipping */
    int32_t sched;                /* GPE_SCHED_* */
    float T_0, T_mult, eta_min;   /* cosine warm restarts (refine/...:312-314) */
    float factor; int32_t patience; float min_lr, threshold;   /* ReduceLROnPlateau (nb c10:L76-78) */
    /* execution */
    int32_t path;                 /* GPE_PATH_* */
    int32_t world_size;           /* data-parallel ranks sharing the replicated boundary batch (>=1) */
    int32_t history_capacity;     /* steps of scalar history kept on device (0: default 65536) */
    /* early stopping, evaluated on the device after every update (refine/...:363-400): stop when loss <= stop_tol or
     * after stop_patience steps without a new best loss; once stopped, further steps leave the parameters untouched.
     * stop_tol <= 0 and stop_patience <= 0 disable the respective test. */
    float stop_tol;
    int32_t stop_patience;
    /* row f3 of SURVEY 8: other bases / hard boundary factor (1D) */
    int32_t base_kind;            /* GPE_BASE_* (used when base_mode >= 0) */
    int32_t envelope;             /* GPE_ENV_* */
    float box_L;                  /* L of the box base */
    float env_L;                  /* L of the sin(pi x / L) factor */
    /* row f4: Riesz energy term  w_riesz * E  (real psi, any dimension), riesz_kind =
     *   GPE_RIESZ_PAPER       E = [1/2 sum |grad u|^2 + sum V u^2 + gamma/(p+1) sum |u|^(p+1)] / sum u^2
     *                         (Notebooks/Paper/Gross_Pitaevskii_1D_Harmonic.ipynb c6:L133-183)
     *   GPE_RIESZ_SUM         E = 1/2 sum |grad u|^2 + 1/2 sum V u^2 + gamma/(p+1) sum |u|^(p+1)   (unnormalised point sums:
     *                         src/gross_pitaevskii_2D.py:112-151, p = 3: 1/2 (K + P + eta/2 sum u^4))
     *   GPE_RIESZ_VARIATIONAL E = energy of the NORMALISED state u/sqrt(I), I = dx sum u^2:
     *                         [c sum |grad u|^2 + sum V u^2] / sum u^2 + 2 gamma/(p+1) sum |u|^(p+1) / (sum u^2 * I^((p-1)/2)).
     *                         Scale-invariant; its stationary points are exactly the solutions of
     *                         -c lap v + V v + gamma |v|^(p-1) v = mu v, int v^2 = 1, and its minimiser is the ground state -- the
     *                         term that keeps training off the excited states without biasing the other loss terms */
    float w_riesz;
    int32_t riesz_kind;
    /* row f3: network flavour.  GPE_NET_RESIDUAL: layers = [d, H, ..., H, out] describes Linear(d,H) + activation, len(layers)-3
     * residual blocks  tanh(lin2(tanh(lin1 x)) + x)  and Linear(H,out) (refine/box_to_gaussian_pinn_simulation.py:52-63,100-130);
     * parameters in state_dict order network.0, network.2.lin1, network.2.lin2, network.3.lin1, ... (generic kernel set) */
    int32_t net_kind;
    int32_t lambda_kind;          /* GPE_LAMBDA_* (ENERGY: real psi, odd p) */
    /* regularisers of the 2D classes' pde_loss (src/gross_pitaevskii_2D.py:197-211 ; arXiv 2010.05075), added to the total loss:
     *   w_reg_f   / (mean(u^2) + reg_f_eps)      "L_f": keeps the network off the trivial eigenfunction (reference: w = 1, eps = 1e-2)
     *   w_reg_lam / (lambda^2 + reg_lam_eps)     "L_lambda": keeps lambda off zero (reference: w = 1, eps = 1e-6; needs GPE_LAMBDA_ENERGY)
     * mean over n_global; both zero: the terms are not formed */
    float w_reg_f, reg_f_eps, w_reg_lam, reg_lam_eps;
    /* Two-component mixture (0 = off): the two outputs are the REAL order parameters u_1, u_2 of a binary condensate in one trap V,
     *   H_a u_a = -c lap u_a + V u_a + (g_a1 u_1^2 + g_a2 u_2^2) u_a,   a = 1, 2,   g_21 = g_12      (layers[last] == 2, p == 3)
     *   mu_a = sum u_a H_a u_a / sum u_a^2 (one Rayleigh quotient per component),   I_a = dx sum u_a^2,   r_a = H_a u_a - mu_a u_a
     *   loss = w_pde sum_m (r_1^2 + r_2^2) / N + w_norm sum_a (I_a - n_a)^2 + w_bc bc      (bc as for complex psi: both outputs, cnt = n_b * 2)
     * Seeds at the output jets, rb_a = 2 w_pde r_a / N, b the other component, mu_a held constant (its branch of the gradient vanishes:
     * d loss / d mu_a = -2 w_pde / N sum r_a u_a = 0):
     *   d/du_a     = rb_a (V + 3 g_aa u_a^2 + g_ab u_b^2 - mu_a) + rb_b 2 g_ab u_a u_b + 4 w_norm (I_a - n_a) dx u_a
     *   d/d(lap u_a) = -c rb_a ;  first-derivative seeds 0 (the energy term adds to both: gpe_mixture_energy_weight, below)
     * gamma, complex_psi, omega_rot, base_mode, envelope, w_sym, w_orth, w_riesz, lambda_kind, the regularisers and residual blocks do
     * not combine with a mixture: gpe_create refuses them.  Quadrature weights, merged boundary rows, the samplers, the pre-training
     * step, gpe_run and the data-parallel entry points work as for any n_out = 2 network; (num_2, den_2) travel in slots 10, 11 of the
     * first exchange message.  gpe_scalars reports component 1 (mu, num, den, integral) and norm = sum_a (I_a - n_a)^2; component 2 is
     * read with gpe_mixture_scalars.  w_riesz is the scalar problem's term; a mixture's own energy term is switched on for the live engine
     * with gpe_mixture_energy_weight and needs no configuration field.  The three fields were appended without a change of GPE_ABI_VERSION: a binding verifies its layout
     * against gpe_sizeof_config(), and a zero-filled tail means "no mixture". */
    int32_t mixture;
    float mix_g[3];               /* g_11, g_22, g_12 */
    float mix_norm[2];            /* target norms n_1, n_2 (> 0) */
} gpe_config;

/* Per-step scalars (refine/...:364-381 keeps loss every 10 and lambda every 100 epochs). */
typedef struct gpe_scalars {
    double loss, pde, bc, norm, sym, orth;
    double mu;                    /* Rayleigh quotient lambda_pde (refine/...:186-188) */
    double num, den, sum_r2, integral;
    double grad_norm, lr;
    double step;                  /* 1-based optimiser step that produced this record */
    double nonfinite;             /* 1 when the loss or gradient was not finite (no update) */
    double riesz;                 /* Riesz energy E (0 when w_riesz == 0) */
    double reg;                   /* w_reg_f / (mean u^2 + eps) + w_reg_lam / (lambda^2 + eps)  (0 when both weights are 0) */
} gpe_scalars;

/* Observables of the state on a point set, formed on the device (gpe_observables, the monitor ring).  Replaces the host-side sums of
 * tools/accuracy_cfg4.py:state_numbers and tools/accuracy_nd.py (jets copied to the host, numpy); the reference has no counterpart:
 * it never evaluates energy, chemical potential or <L_z> of a trained state.
 * u is the physical wavefunction as the head forms it (envelope, perturb_scale, analytic base included), c = kinetic_coeff, dv the
 * quadrature weight, I = dv sum |u|^2.  With K = c dv sum |grad u|^2, P = dv sum V |u|^2, S = dv sum Re(u* N(u)) (N the engine's nonlinear
 * term: gamma u^p, gamma |u|^(p-1) u under abs_power, gamma |psi|^2 psi for complex psi, where p counts as 3) and
 * L = dv sum [psi_r D psi_i - psi_i D psi_r], D = x d_y - y d_x  (-Omega L_z psi = i Omega D psi):
 *   kin = K/I, pot = P/I, inter = 2/(p+1) S / I^((p+1)/2), rot = -Omega L/I, lz = L/I
 * -- the energy of the NORMALISED state u/sqrt(I), the formulas of GPE_RIESZ_VARIATIONAL above.  Sums in fp64 from the fp32 jets, added
 * in a fixed order (no atomics): a record repeats bit for bit.  Single-rank semantics: every rank of a data-parallel run gets the
 * numbers of its own points; combining ranks is left to the caller.
 * (The struct has no typedef of its own name: C keeps typedef names and functions in one name space, and the entry point is called
 * gpe_observables.  Write `struct gpe_observables`.) */
struct gpe_observables {
    double n, dv, step;          /* points, quadrature weight, optimiser step of the parameters evaluated (device-side value) */
    double norm;                 /* I = dv * sum |u|^2 of the RAW state */
    double kin, pot, inter, rot; /* energy parts of the NORMALISED state u / sqrt(I) */
    double energy;               /* kin + pot + inter + rot */
    double mu;                   /* kin + pot + (p+1)/2 * inter + rot */
    double mu_lap;               /* mu with the kinetic part taken as -c * dv * sum Re(u* lap u) / I instead of kin */
    double lz;                   /* <L_z> of the normalised state (0 for real psi) */
    double mean_x[3], var_x[3];  /* density-weighted centre and variance per axis (unused axes 0) */
    double peak_density;         /* max |u|^2 / I */
    double res_rms;              /* sqrt(dv * sum |H[phi] phi - mu phi|^2), phi = u / sqrt(I): the residual of the normalised state (two-pass) */
};

/* Observables of a two-component mixture state on a point set, formed on the device (gpe_mixture_observables, the mixture monitor's
 * ring, the mixture keeper's record).  Replaces the host-side sums of tools/accuracy_mixture.py:state (jets copied to the host, numpy);
 * the reference has no counterpart.  u_a are the two real order parameters as k_head_mix forms them (perturb_scale included),
 * c = kinetic_coeff, dv the quadrature weight, (n_1, n_2) = mix_norm, (g_11, g_22, g_12) the couplings in force at the call.  Raw point
 * sums (times q_i on the bound set under gpe_bind_weights):
 *   s_a = sum u_a^2,  K_a = sum |grad u_a|^2,  P_a = sum V u_a^2,  L_a = sum u_a lap u_a,  Q_ab = sum u_a^2 u_b^2,   I_a = dv s_a
 * Every field but `norm` describes the state NORMALISED TO THE TARGET NORMS, v_a = u_a sqrt(n_a / I_a) -- the convention of the mixture
 * energy term (gpe_mixture_energy_weight): `energy` is that term's E with dx = dv, and no field changes when a component is scaled.
 * All doubles, at most 64 of them (the keeper files one double per lane of a wave).  Sums in fp64 from the fp32 jets, added in a fixed
 * order (no atomics): a record repeats bit for bit.  Single-rank semantics, as struct gpe_observables.
 * (No typedef of its own name, for the reason given there: write `struct gpe_mixture_observables`.) */
struct gpe_mixture_observables {
    double n, dv, step;          /* points, quadrature weight, optimiser step of the parameters evaluated (device-side value) */
    double norm[2];              /* I_a of the RAW state */
    double kin[2];               /* c n_a K_a / s_a */
    double pot[2];               /* n_a P_a / s_a */
    double inter[3];             /* (11, 22, 12): 1/2 g_11 n_1^2 Q_11 / (s_1^2 dv), 1/2 g_22 n_2^2 Q_22 / (s_2^2 dv), g_12 n_1 n_2 Q_12 / (s_1 s_2 dv) */
    double energy;               /* the sum of the seven fields above */
    double mu[2];                /* c K_a/s_a + P_a/s_a + g_aa n_a Q_aa / (s_a^2 dv) + g_12 n_b Q_12 / (s_1 s_2 dv), b the other component;
                                  * sum_a n_a mu_a = energy + inter[0] + inter[1] + inter[2] */
    double mu_lap[2];            /* mu with the kinetic part taken as -c L_a / s_a */
    double overlap;              /* Q_12 / sqrt(Q_11 Q_22): 0 when phase-separated, 1 when the densities are proportional */
    double mean_x[2][3], var_x[2][3];   /* density-weighted centre and variance per component and axis (unused axes 0) */
    double peak_density[2];      /* n_a max u_a^2 / I_a */
    double res_rms[2];           /* sqrt(dv sum |H_a[v] v_a - mu_a v_a|^2): the residual of the normalised state (two-pass) */
    double res_rms_total;        /* sqrt(res_rms[0]^2 + res_rms[1]^2) */
};

/* ---- lifetime ------------------------------------------------------------------------------ */
int gpe_abi_version(void);
size_t gpe_sizeof_config(void);   /* sizeof(gpe_config)  -- lets a foreign-language binding verify its struct layout */
size_t gpe_sizeof_scalars(void);  /* sizeof(gpe_scalars) */
size_t gpe_sizeof_observables(void);   /* sizeof(struct gpe_observables) */
size_t gpe_sizeof_mixture_observables(void);   /* sizeof(struct gpe_mixture_observables) */
/* replaces: GrossPitaevskiiPINN(...).to(device) + torch.optim.Adam(...) + scheduler construction
 * (refine/harmonic_pinn_simulation.py:295,309-314 ; nb c10:L63,L73-78) */
int gpe_create(const gpe_config* cfg, int device, void* hip_stream, gpe_engine** out);
void gpe_destroy(gpe_engine* e);
const char* gpe_last_error(const gpe_engine* e); /* e may be NULL: last create() error */
/* 1 = generic kernels, 2 = fused MFMA kernels (what gpe_create selected) */
int gpe_active_path(const gpe_engine* e);
/* "fwd=<kernel>;bwd=<kernel>": the jet forward / reverse kernels the bound collocation batch is dispatched to (the engine
 * picks among several by shape, batch size and the GPE_* tuning switches).  Needs gpe_bind_points first. */
int gpe_active_kernels(gpe_engine* e, char* buf, size_t n);

/* ---- parameters: model.state_dict() / load_state_dict() (refine/...:299,909,953) --------------- */
/* Hidden widths: the MFMA kernel sets exist for one width of 32, 64, 128 or 256 (>= 2 hidden layers).  An MLP with other hidden widths <= 256 is
 * run padded to the next of those with units that output exactly 0 (zero weights; bias 0 for tanh, -40 for tanh + 1): the same function and
 * gradients, and the padding does not move under Adam.  Every call below takes and returns the network AS GIVEN in gpe_config.layers.
 * Residual blocks, widths above 256 and single-hidden-layer networks run on the generic layer-by-layer kernel set (widths above 256 padded to a
 * multiple of 256 for its MFMA kernels). */
int64_t gpe_param_count(const gpe_engine* e);
int gpe_set_params(gpe_engine* e, const float* h_flat, size_t n);
int gpe_get_params(gpe_engine* e, float* h_flat, size_t n);
int gpe_get_grad(gpe_engine* e, float* h_flat, size_t n);            /* gradient of the last step (after exchange, before clipping) */
int gpe_get_adam_state(gpe_engine* e, float* h_m, float* h_v, size_t n, int64_t* step);
int gpe_set_adam_state(gpe_engine* e, const float* h_m, const float* h_v, size_t n, int64_t step);
int gpe_reset_optimizer(gpe_engine* e, float lr);                    /* new Adam + scheduler state (refine/...:309-314 per gamma) */

/* ---- data binding: X_tensor, boundary_points (refine/...:260-264) ----------------------------------- */
/* d_x [n_local, dim] row-major fp32; d_V [n_local] or NULL (precomputed_potential, refine/...:146,175-178).
 * GPE_POT_PRECOMPUTED needs d_V -- unless terms are bound (gpe_potential_terms): then d_V must be NULL and the engine fills its own V.
 * Buffers stay owned by the caller and must outlive their use. */
int gpe_bind_points(gpe_engine* e, const float* d_x, int64_t n_local, const float* d_V);
int gpe_bind_boundary(gpe_engine* e, const float* d_xb, int64_t n_b, const float* d_target /* [n_b,out] or NULL = 0 */);
int gpe_bind_orth(gpe_engine* e, int k, const float* d_psi_k /* [n_local] or NULL to clear (a caller array or a frozen state) */);
/* Frozen reference state in orthogonality slot k (0 .. GPE_MAX_ORTH-1): a parameter set of the engine's OWN network (layers,
 * activation, net_kind; caller's layout as gpe_set_params, n == gpe_param_count) that the engine keeps on the device and evaluates
 * itself:  psi_k(x) = amplitude * ( env(x) * perturb_scale * NN_theta_k(x) + phi_{base_mode}(x) )
 * base_mode < 0: no base.  Base kind / envelope are the engine's.  h_flat == NULL clears the slot.  A slot holds a caller array
 * (gpe_bind_orth) or a frozen state; binding one kind replaces the other.  psi_k lives in an engine-owned buffer [n_local] that the
 * head / seed kernels read like a caller's array; it is filled on the engine's stream -- here (if points are bound), at every
 * gpe_bind_points / gpe_bind_sampler, and directly behind every redraw of the sampler -- by the forward pass behind gpe_forward run
 * on the frozen parameters (same kernel set, width padding and weight packing as the trained ones) and one elementwise kernel.
 * Never part of a captured graph.  Later gpe_set_params / gpe_set_perturb_scale / gpe_set_gamma / gpe_reset_optimizer do not touch it.
 * Every step entry point honours it (gpe_step, gpe_run, the three phases, gpe_step_dp / gpe_run_dp: each rank fills its own rows).
 * GPE_ERR_INVALID: complex psi or out != 1, n != gpe_param_count, k out of range, base_mode >= 0 with GPE_BASE_PRECOMPUTED or dim > 1,
 * perturb_scale / amplitude not finite.  A bind that fails leaves the slot as it was.
 * Replaces: the host-side evaluate-and-upload a caller of gpe_bind_orth needs per point set (no reference counterpart). */
int gpe_bind_orth_state(gpe_engine* e, int k, const float* h_flat, size_t n, int base_mode, float perturb_scale, float amplitude);
/* synchronise; the engine-owned array psi_k [n] on the collocation set bound now.  GPE_ERR_STATE: slot k holds no frozen state, or no points bound. */
int gpe_orth_values(gpe_engine* e, int k, const float** d_psi, int64_t* n);
/* GPE_BASE_PRECOMPUTED: phi, phi', phi'' of the base on the bound points, each [n_local].  The boundary term then uses no
 * base: fold phi(x_b) into the boundary target. */
int gpe_bind_base(gpe_engine* e, const float* d_phi, const float* d_phi1, const float* d_phi2);

/* ---- device-side stratified collocation sampler --------------------------------------------------------------------------------
 * One uniformly placed point per cell of a regular grid, re-drawn in place every `every` steps by a kernel on the engine's stream:
 * no host synchronisation, no pointer change (a captured graph stays valid), and any set is a pure function of (seed, draw, cell).
 * Replaces the host loop of tools/accuracy_nd.py:run_epochs (16 jittered numpy copies of the grid, uploaded and cycled through
 * gpe_bind_points); the reference has no counterpart: it trains on one fixed grid.
 *   grid   axis k has shape[k] cells over [lo[k], hi[k]], h[k] = float((double(hi[k]) - double(lo[k])) / shape[k]); axes beyond the
 *          network's input dimension have shape 0.  Cells are numbered row-major, last axis fastest (np.meshgrid(indexing="ij")
 *          ravelled); row j of the local batch is cell first_cell + j, so ranks holding contiguous blocks hold the world-1 set.
 *   words  Philox4x32-10, counter (cell & 0xffffffff, cell >> 32, draw & 0xffffffff, draw >> 32), key (seed & 0xffffffff, seed >> 32),
 *          one call per point, output word k for axis k.
 *   point  u = float(r >> 8) * 2^-24;  t = float(i_k) + u;  x = lo[k] + t * h[k] (one rounded fp32 multiply, one rounded fp32 add,
 *          never an fma);  x = min(max(x, clip_lo[k]), clip_hi[k]).  gpe_pinn/sampler.py restates this in numpy, bit for bit.
 *   when   draw0 at the bind; enqueued steps s (counted on the host since the bind, as the monitor counts) with
 *          m * every <= s < (m + 1) * every run on draw draw0 + m; the redraw is enqueued before the first kernel of step m * every. */
typedef struct gpe_sampler_spec {
    int64_t shape[3];
    float lo[3], hi[3], clip_lo[3], clip_hi[3];
    uint64_t seed;
    int64_t first_cell, n_local, draw0, every;
} gpe_sampler_spec;
size_t gpe_sizeof_sampler_spec(void);   /* sizeof(gpe_sampler_spec) */
/* Allocates the engine-owned point buffer [n_local, dim], draws draw0 into it and binds it as the collocation batch with no potential
 * array (and the [x ; -x] symmetry batch when w_sym != 0, refreshed by every redraw).  Every step entry point honours the sampler:
 * gpe_step, gpe_run (which cuts its graph replays at redraw steps), gpe_step_dp, gpe_run_dp and the three-phase gpe_step_begin.
 * spec == NULL clears the sampler and leaves no points bound.  GPE_ERR_INVALID: GPE_POT_PRECOMPUTED without bound terms or GPE_BASE_PRECOMPUTED (their arrays
 * would be stale; with gpe_potential_terms the engine owns V and refills it behind every draw), a caller's orthogonality array bound (frozen states of gpe_bind_orth_state are fine), every <= 0, hi <= lo or clip_hi < clip_lo on a used axis, first_cell + n_local beyond
 * the product of shape, axes used other than the network's input dimension.  While a sampler is bound gpe_bind_orth with an array,
 * gpe_bind_target and the gpe_mse_* entry points return GPE_ERR_STATE (their arrays live on fixed points); gpe_bind_points clears
 * the sampler and the caller's points take over.
 * Replaces: the host loop of tools/accuracy_nd.py:run_epochs (no reference counterpart). */
int gpe_bind_sampler(gpe_engine* e, const gpe_sampler_spec* spec);
/* synchronise; the engine-owned buffer d_x [n, dim], and the draw index of the set it holds now.  Any of the three may be NULL.
 * Replaces: reading back the bound set in tools/accuracy_nd.py:run_epochs (the host there built it; no reference counterpart). */
int gpe_sampler_points(gpe_engine* e, const float** d_x, int64_t* n, int64_t* draw);

/* ---- per-point quadrature weights -------------------------------------------------------------------------------------------------
 * d_q [n_local] fp32 on the device, one weight q_i >= 0 per bound collocation row, caller-owned like d_V.  While weights are bound
 *   sums   every sum over collocation points takes the factor q_i: num, den, the orthogonality overlaps, the Riesz / energy sums, sum r^2
 *   means  every N of a mean becomes W = sum q_i over ALL ranks: w_pde sum q r^2 / W, the 2 w_pde / W of the seeds, the energy-lambda
 *          branch, w_reg_f / (sum q u^2 / W + eps).  gpe_config.dx stays the plain multiplier it is (I = dx sum q u^2, overlaps
 *          dx sum q psi_k u): a caller whose q_i are cell volumes sets dx = 1
 *   seeds  dLoss / d(output jets of row i) = the unweighted expression with N -> W, times q_i; a row with q_i = 0 contributes nothing
 *   rows   boundary rows riding in the batch and the separate boundary batch have no weight
 *   gpe_scalars.num / den / sum_r2 / integral report the weighted sums.
 * With integer weights the step equals the unweighted step on the batch with row i repeated q_i times and n_global = sum q.
 * The step then forms head and seeds with the weighted instances of the standalone kernels (k_head_pde / k_seed_pde), at every batch
 * size: the fused head / seed code of the small-batch kernels has no weights (gpe_active_kernels names them: ";head=...;seed=...").
 * gpe_observables on the bound set (d_x == NULL) honours the weights: every sum takes q_i, dv stays the multiplier, peak_density stays
 * the plain maximum, n the row count.  An explicit d_x, the monitor and the gpe_mse_* pre-training loss are and stay unweighted.
 * The bind reduces the array once (one kernel, fp64, fixed order, no atomics) and synchronises once: w_local = sum q_i of this rank.
 * w_total > 0: the caller's W over all ranks (data-parallel runs); 0: W = w_local.  d_q == NULL clears the weights and restores the
 * count-based N.  gpe_bind_points and gpe_bind_sampler clear bound weights (weights belong to rows).  While weights are bound
 * gpe_set_n_global returns GPE_ERR_STATE and gpe_set_loss_weights with w_sym != 0 GPE_ERR_INVALID.  A captured graph is rebuilt after
 * a bind or a clear, as after a bind of points.
 * GPE_ERR_INVALID: a negative or non-finite entry, w_local == 0, w_total negative or not finite, w_sym != 0 (the symmetry batch has no
 * weights).  GPE_ERR_STATE: no points bound, or a sampler bound (its rows move; d_q == NULL under a graded sampler, which owns its
 * weights, too).  A bind that fails leaves what was there.
 * Replaces: nothing a caller could do host-side -- without weights every training set had to be a uniform grid (the reference's 2D
 * prepare_training_data draws a polar set and weights nothing: src/gross_pitaevskii_2D.py). */
int gpe_bind_weights(gpe_engine* e, const float* d_q, double w_total);
/* synchronise; the array the step reads (the caller's, or the graded sampler's own), its length, sum q_i of this rank and W.  Any out
 * pointer may be NULL.  GPE_ERR_STATE: no weights bound.
 * Replaces: the caller's own bookkeeping of sum q (and, under a graded sampler, rebuilding the cell volumes on the host). */
int gpe_weights(gpe_engine* e, const float** d_q, int64_t* n, double* w_local, double* w_total);
/* Graded stratified sampler: gpe_bind_sampler on a tensor-product grid with caller-given, non-uniform cell edges -- one uniformly
 * placed point per cell, weighted by its cell's volume.  spec as for gpe_bind_sampler (shape, clip_*, seed, first_cell, n_local, draw0,
 * every mean what they mean there); h_edges{k}: HOST array of shape[k] + 1 strictly increasing finite floats per used axis (NULL for
 * the others), copied to the device here; spec.lo[k] / hi[k] must equal the first / last edge.
 *   point   cell i of axis k: a = edges_k[i], b = edges_k[i + 1], w = b - a (one rounded fp32 subtraction), u as above,
 *           x = a + u * w (one rounded multiply, one rounded add, never an fma), then the clip by comparisons
 *   weight  q = w_0, then q * w_1, then * w_2: rounded fp32 multiplies in axis order; written once at the bind (no draw changes it)
 *   W       product over the axes of the fp64 sums, in index order, of the fp32 widths -- of the WHOLE grid, not of this rank's block
 * gpe_pinn/sampler.py (graded_points, graded_weights, graded_total) restates all three, bit for bit.  The bind allocates the engine-owned
 * point buffer and an engine-owned weight buffer [n_local], draws draw0, and binds both (as gpe_bind_weights with w_total = W).  Cadence,
 * graph cutting, gpe_sampler_points, the refill of frozen orthogonality states behind every redraw and the data-parallel / three-phase
 * entry points behave as with the uniform sampler.  gpe_bind_sampler(NULL) and gpe_bind_points clear it, weights included.
 * GPE_ERR_INVALID: whatever gpe_bind_sampler refuses, edges that are missing, not finite or not strictly increasing, lo / hi other than
 * the end edges, w_sym != 0.
 * Replaces: a host loop that redraws a graded set, recomputes nothing but uploads points every K steps (no reference counterpart). */
int gpe_bind_sampler_graded(gpe_engine* e, const gpe_sampler_spec* spec, const float* h_edges0, const float* h_edges1, const float* h_edges2);
/* Residual-adaptive sampler: the cells of a graded grid become BLOCKS, and a buffer of n_points = N rows (a fixed count: buffers, pointers,
 * kernel selection and a captured graph stay valid) is shared out among them anew at every redraw, by the PDE residual of the state
 * being trained.  spec, h_edges{k} as for gpe_bind_sampler_graded; B = prod(shape) blocks, row-major, last axis fastest; v_b = the graded
 * sampler's fp32 cell volume, V its W.  Single-rank: spec.first_cell = 0, spec.n_local = B.
 *   rows    block b holds rows [off_b, off_{b+1}), off the exclusive prefix sum of the counts n_b; row j lies in block
 *           b = upper_bound(off, j) - 1 with local index l = j - off_b
 *   point   Philox4x32-10, counter (b, l, draw & 0xffffffff, draw >> 32), key as above, output word k for axis k; u, w, x = a + u * w and
 *           the clip per axis exactly as gpe_bind_sampler_graded
 *   weight  q = float(double(v_b) / double(n_b)) for every row of block b: one IEEE fp64 division, one conversion.  W = V, constant
 *   masses  directly before redraw m >= 1 (enqueued before the first kernel of step m * every) the engine evaluates the residual of the
 *           current parameters on the set it holds, with that set's weights, by the forward-only launches of gpe_residual -- without a
 *           host synchronisation and without writing anything a step reads (optimiser state, scheduler, history, `last`, stop flag) --
 *           and forms m_b = sum_{i in b} q_i sum_c r_{i,c}^2 and M = sum_b m_b in fp64, each in a fixed order, no atomics
 *   counts  ok = M > 0 && M < inf;  kA_b = ok ? uint64(floor(m_b / M * 2^30)) : 0;  kV_b = uint64(floor(double(v_b) / V * 2^30));
 *           k_b = (1024 - s) kA_b + s kV_b with s = uniform_per_1024, the share always allocated by volume (no block starves);
 *           K the exclusive prefix sum of k;  R = N - B n_min;  n_b = n_min + (K_{b+1} R) / K_B - (K_b R) / K_B in unsigned 64-bit
 *           integer division.  The counts add up to N exactly; a zero or non-finite mass anywhere gives the allocation by volume, and so
 *           does the bind (draw0: all masses zero, no forward pass, nothing trained needed).
 * gpe_pinn/sampler.py (adaptive_counts, adaptive_points, adaptive_weights) restates counts, points and weights, bit for bit.  The bind
 * allocates every buffer (points, weights, residual, masses, counts, offsets); a redraw allocates and synchronises nothing.  Cadence,
 * graph cutting (gpe_run), gpe_step / gpe_step_begin, gpe_sampler_points, gpe_weights (w_total = V; w_local = the sum of the bind's
 * weights), the refill of frozen orthogonality states behind every redraw, the monitor and the keeper behave as with the graded
 * sampler.  gpe_bind_sampler(NULL) and gpe_bind_points clear it; gpe_bind_weights returns GPE_ERR_STATE while it is bound.
 * GPE_ERR_INVALID: whatever gpe_bind_sampler_graded refuses (w_sym != 0 included), n_points > 2^22 (the products above stay below
 * 2^63; hence B <= 2^22), B * n_min > n_points, n_min < 1, uniform_per_1024 outside [1, 1024], first_cell != 0 or n_local != B.
 * GPE_ERR_STATE: the engine has a communicator; with an adaptive sampler bound gpe_comm_init, gpe_step_dp and gpe_run_dp return it
 * too (a data-parallel allocation needs a mass exchange).
 * Replaces: a host loop of gpe_residual, a per-block sum, an allocation and gpe_bind_points + gpe_bind_weights every K steps, with
 * its synchronisations and uploads (residual-based adaptive sampling: Wu et al. 2023; the reference trains on one fixed grid). */
int gpe_sampler_adaptive(gpe_engine* e, const gpe_sampler_spec* spec, const float* h_edges0, const float* h_edges1, const float* h_edges2,
                         int64_t n_points, int32_t n_min, int32_t uniform_per_1024);
/* synchronise; the block masses h_mass [B] and their total M that produced the counts of the set held now (all zero after the bind), those
 * counts h_count [B] and the draw index.  Host arrays; any pointer may be NULL.  GPE_ERR_STATE: no adaptive sampler bound.
 * Replaces: the host's own record of its last allocation in the loop named above. */
int gpe_sampler_adaptive_state(gpe_engine* e, double* h_mass /*[B]*/, double* mass_total, int32_t* h_count /*[B]*/, int64_t* draw);
/* B and N of the adaptive sampler bound now: what a caller sizes h_mass / h_count by.  No synchronisation (both are host-side facts of
 * the bind); either pointer may be NULL.  GPE_ERR_STATE: no adaptive sampler bound.
 * Replaces: the caller remembering prod(shape) of its own bind. */
int gpe_sampler_adaptive_blocks(gpe_engine* e, int64_t* n_blocks, int64_t* n_points);
/* Cell-subset sampler: the uniform or the graded stratified sampler on a SUBSET of the grid's cells -- a disk, a ball, an annulus, any
 * mask -- so that rows which would carry nothing are never launched.  spec.shape / lo / hi / clip_* / seed / draw0 / every mean what they
 * mean for gpe_bind_sampler; h_cells [n_cells]: HOST array, the global list of kept cells as row-major indices of that grid (last axis
 * fastest), strictly ascending, copied to the device here and owned by the engine (its pointer stays until the next bind of a sampler
 * or of points).  spec.first_cell / n_local index the LIST: this engine holds rows [first_cell, first_cell + n_local) of it, so ranks
 * holding contiguous blocks of the list hold, together, the world-1 set.
 *   rows    row j of the local batch is cell c = h_cells[first_cell + j]
 *   point   Philox4x32-10, counter (c & 0xffffffff, c >> 32, draw & 0xffffffff, draw >> 32), key (seed & 0xffffffff, seed >> 32), output
 *           word k for axis k; everything behind it exactly as gpe_bind_sampler (all h_edges NULL: the uniform grid) or as
 *           gpe_bind_sampler_graded (h_edges{k} given for every used axis): the row holds the bits row c of the full grid's set holds
 *   uniform no weights are bound and the step runs on the kernels of gpe_bind_sampler (gpe_active_kernels is unchanged); the caller sets
 *           gpe_config.dx to the cell volume and n_global to n_cells
 *   graded  the rows get their cells' fp32 volumes as weights, as gpe_bind_sampler_graded binds them (set dx = 1): w_local = the fp64 sum
 *           over this engine's rows; w_total = W = the fp64 sum, in list order, over the WHOLE list of the same fp32 volumes, formed on
 *           the host at the bind.  gpe_weights reports both
 *   when    draw0 at the bind; the redraw is enqueued before the first kernel of step m * every, counted on the host since the bind, as
 *           for gpe_bind_sampler
 * gpe_pinn/sampler.py (cells_points, cells_weights, cells_total; ball_cells / mask_cells build lists) restates all of it, bit for bit.
 * gpe_step, gpe_run and its graph cutting, gpe_step_begin, gpe_step_dp / gpe_run_dp, gpe_sampler_points, the refill of frozen
 * orthogonality states behind every redraw, the monitor, the keeper and the mixture engines behave as with the uniform / graded
 * sampler.  It replaces a sampler of any other kind and any other replaces it; gpe_bind_sampler(NULL) and gpe_bind_points clear it, list and
 * weights included.  While it is bound gpe_bind_orth with an array, gpe_bind_target, the gpe_mse_* and gpe_lbfgs_* entry points and
 * gpe_bind_weights answer as for any sampler with every > 0.
 * GPE_ERR_INVALID, each leaving the engine as it was: whatever gpe_bind_sampler refuses (with first_cell + n_local held to n_cells);
 * h_cells NULL or n_cells <= 0; a list that is not strictly ascending (the message names the first offending position); a cell outside
 * [0, prod shape); edges given for some used axes but not all; whatever gpe_bind_sampler_graded refuses of edges, lo / hi and w_sym.
 * Replaces: the corner cells of tools/accuracy_nd.py's box, which a radially trapped state leaves empty (--ball), and, for any problem
 * whose potential the engine evaluates itself, a host-side draw on a disk like the reference's prepare_training_data
 * (src/gross_pitaevskii_2D.py).  Not the 2D classes of gpe_pinn/surface.py themselves: their two-dimensional Gaussian potential is fed as
 * GPE_POT_PRECOMPUTED (GPE_POT_GAUSSIAN is the notebook's exp(-(x - a)^2) along x), which a sampler takes once the well is bound as a
 * GPE_TERM_GAUSS term (gpe_potential_terms) and refuses as a caller's array. */
int gpe_sampler_cells(gpe_engine* e, const gpe_sampler_spec* spec, const int64_t* h_cells, int64_t n_cells,
                      const float* h_edges0, const float* h_edges1, const float* h_edges2);
/* synchronise; the engine-owned DEVICE copy of the list, its length and this engine's first row in it.  Any out pointer may be NULL.
 * GPE_ERR_STATE: no cell-subset sampler bound.
 * Replaces: the caller keeping its own copy of the list it bound. */
int gpe_sampler_cells_read(gpe_engine* e, const int64_t** d_cells, int64_t* n_cells, int64_t* first);

/* ---- analytic potential terms: any trap on sampler-drawn sets -------------------------------------------------------------------------
 * The engine evaluates three potentials inside its kernels (GPE_POT_HARMONIC / GAUSSIAN / PERIODIC); every other one is an array on fixed
 * points (GPE_POT_PRECOMPUTED).  With a TABLE OF TERMS bound, an engine configured GPE_POT_PRECOMPUTED owns that array: one small kernel
 * (csrc/gpe_potential.h: k_potential_terms) fills it on the engine's stream at every bind of points and directly behind every redraw of a
 * sampler -- before the frozen orthogonality states are refilled and before the step's first kernel -- and the step runs on the
 * precomputed-potential path every kernel family already has.  No forward, head, seed or reverse kernel knows of the table.
 *   t_k = w_k (x_k - c_k) for k < dim;  s = sum_k t_k^2, accumulated as s = fmaf(t_k, t_k, s) in ascending k (the arithmetic of the
 *   harmonic case: one QUAD term with a = pot_scale, w = omega, c = (pot_a, 0, 0) gives GPE_POT_HARMONIC's V bit for bit)
 *   GPE_TERM_QUAD     a s                     anisotropic harmonic trap, any centre
 *   GPE_TERM_QUARTIC  a s s                   quartic confinement (fast rotation)
 *   GPE_TERM_GAUSS    a expf(-s)              d-dimensional bump, dimple or (a < 0) well
 *   GPE_TERM_LATTICE  a sum_{k: w_k != 0} cosf(t_k)^2      optical lattice along the axes with w_k != 0
 *   GPE_TERM_LINEAR   a sum_k t_k             tilt, gravity
 *   V(x) = sum_j term_j(x), fp32, added in table order starting from 0.f.  gpe_pinn/potential.py restates it in numpy (fp64: the reference). */
#define GPE_MAX_POT_TERMS 16
enum { GPE_TERM_QUAD = 0, GPE_TERM_QUARTIC = 1, GPE_TERM_GAUSS = 2, GPE_TERM_LATTICE = 3, GPE_TERM_LINEAR = 4 };
typedef struct gpe_pot_term {
    int32_t kind;                 /* GPE_TERM_* */
    float a;
    float w[3], c[3];             /* axes beyond the network's input dimension: 0 */
} gpe_pot_term;                   /* 32 bytes */
/* Copies the table into the engine (n_terms in 1 .. GPE_MAX_POT_TERMS).  On a live engine V of the bound set -- where the engine owns it --
 * and of a monitor set the engine evaluates are refilled, enqueued on the compute stream in stream order with no host synchronisation;
 * the buffers stay where they are, so a captured step graph stays valid: only contents move.  A set bound earlier with a caller's d_V
 * stays on that array.  With terms bound
 *   gpe_bind_points      takes d_V == NULL: the engine allocates V [n_local], fills it and binds it; a d_V is GPE_ERR_INVALID
 *   the four samplers    are accepted on a GPE_POT_PRECOMPUTED engine: V lives beside the point buffer and is refilled behind every draw
 *                        (gpe_step, gpe_run and its graph cutting, gpe_step_begin, gpe_step_dp / gpe_run_dp on each rank's block; the
 *                        adaptive sampler's residual detour runs on the held set, whose V is still the held set's)
 *   gpe_observables, gpe_mixture_observables, gpe_bind_monitor, gpe_mixture_monitor      take d_V == NULL on any point set: the monitor
 *                        gets an engine-owned V for its set, filled at its bind and at every change of the terms; a one-off call fills a scratch V
 * terms == NULL clears the table: GPE_ERR_STATE while a sampler is bound or a monitor holds an engine-evaluated V; otherwise points bound
 * with the engine's V become unbound, as gpe_bind_sampler(NULL) leaves them.  Data-parallel runs: every rank binds the same table, nothing
 * is exchanged.  Checkpoints do not store the table.
 * GPE_ERR_INVALID: the engine's potential is not GPE_POT_PRECOMPUTED, n_terms out of range, an unknown kind, a non-finite a / w / c, a
 * non-zero w_k or c_k on an axis k >= dim, a LATTICE term with every w_k == 0.  A call that fails leaves the table that was there.
 * Replaces: the host-side evaluate-and-upload of V per point set (no reference counterpart: it trains on one fixed grid). */
int gpe_potential_terms(gpe_engine* e, const gpe_pot_term* terms, int32_t n_terms);
/* the bound table: up to GPE_MAX_POT_TERMS records into terms_out (may be NULL), their count into *n_out (0: none bound) */
int gpe_potential_terms_read(gpe_engine* e, gpe_pot_term* terms_out, int32_t* n_out);
/* synchronise; the engine-owned V [n] the bound collocation set runs on.  GPE_ERR_STATE: no terms bound, no points bound, or the bound
 * set runs on a caller's array. */
int gpe_potential_values(gpe_engine* e, const float** d_V, int64_t* n);
/* the fill kernel on any caller points: d_V_out[i] = V(d_x[i, :]), d_x [n, dim]; synchronises.  GPE_ERR_STATE: no terms bound. */
int gpe_potential_eval(gpe_engine* e, const float* d_x, int64_t n, float* d_V_out);

/* ---- forward-only entry points ---------------------------------------------------------------- */
/* model.forward(x) (refine/...:121-125): d_out [n, out] row-major */
int gpe_forward(gpe_engine* e, const float* d_x, int64_t n, float* d_out);
/* NN output jets [C][n][out] (replaces the two torch.autograd.grad calls of refine/...:158-172 at the NN output) */
int gpe_forward_jets(gpe_engine* e, const float* d_x, int64_t n, float* d_jets);
/* pde_loss (refine/...:146-196 ; nb c6:L81-127) + boundary/normalisation/symmetry terms on the bound data,
 * no parameter update.  d_psi [n_local,out], d_residual [n_local,out] may be NULL.  Single-rank semantics. */
int gpe_residual(gpe_engine* e, gpe_scalars* out, float* d_psi, float* d_residual);
/* plot_wavefunction normalisation (refine/...:463-474 ; nb c12:L30-42): u = base + scale*NN on the grid d_x,
 * u /= sqrt(sum u^2 * dx), |u| if abs_flag; d_u [n,out], d_density [n] (either may be NULL) */
int gpe_eval_density(gpe_engine* e, const float* d_x, int64_t n, float dx, int abs_flag, float* d_u, float* d_density);

/* ---- observables of the current state, on the device (replaces tools/accuracy_cfg4.py:state_numbers; no reference counterpart) ------
 * gpe_observables: jets of the current parameters on d_x [n, dim] (the forward pass behind gpe_forward_jets, one allocation of that
 * size: n is not cut into chunks), two reduction passes, synchronise, fill *out.  d_x == NULL: the bound collocation points and their
 * bound potential (d_V, n ignored).  d_V [n]: needed exactly where gpe_bind_points needs it (GPE_POT_PRECOMPUTED; NULL with terms bound).  A precomputed base
 * exists on the bound points only: other point sets are refused with GPE_ERR_INVALID.  dv: quadrature weight. */
int gpe_observables(gpe_engine* e, const float* d_x, int64_t n, const float* d_V, float dv, struct gpe_observables* out);
/* Held-out monitor: after every `every`-th step enqueued since this call by gpe_step / gpe_run, the observables of the parameters
 * that step left behind are evaluated on d_x and appended to a device ring of `capacity` records (<= 0: 4096) -- no host
 * synchronisation, no host copy; the monitor writes nothing a step reads, so the training trajectory is the one without it.
 * The cadence counts ENQUEUED steps (the host has no mirror of the optimiser step: early stopping is decided on the device);
 * the record's `step` field is read on the device.  gpe_run cuts its graph replays at monitor steps and fills in with plain
 * launches.  d_x == NULL or every <= 0 clears the monitor.  A bind that fails leaves the monitor that was there, its records
 * included.  With a precomputed base (monitor on the bound points only) gpe_bind_points and gpe_bind_base clear the monitor.
 * Buffers stay the caller's.  gpe_step_dp / gpe_run_dp and the
 * three-phase entry points ignore the monitor. */
int gpe_bind_monitor(gpe_engine* e, const float* d_x, int64_t n, const float* d_V, float dv, int64_t every, int32_t capacity);
/* synchronise; *available = records written since the bind; copies records [first, first+count) (0-based since the bind) to out.
 * Only the newest `capacity` records survive: an older one is GPE_ERR_INVALID.  count == 0 with out == NULL just asks. */
int gpe_read_monitor(gpe_engine* e, int64_t first, int64_t count, struct gpe_observables* out, int64_t* available);

/* ---- keeper: the best parameters by the held-out monitor, kept on the device, and a patience stop (no reference counterpart: the
 * reference returns what its last epoch left, and its early stop, refine/...:389-400, watches the training loss) -----------------------
 * Replaces the host loop gpe_run(every) / gpe_read_monitor / gpe_get_params / compare, which costs a synchronisation and a copy of all
 * parameters per monitor step.  Directly behind every monitor record two kernels run on the engine's stream (never captured, nothing
 * synchronises, nothing is allocated): with m the chosen field of the record and best = +inf at the start,
 *   the record IMPROVES iff  isfinite(m) && m < best - min_delta     (lower is better; a tie or a non-finite m does not)
 *   on improvement: best = m, the record and the parameters are copied aside, since_best = 0; otherwise since_best += 1
 *   patience > 0 and since_best >= patience and not yet stopped: the optimiser stops exactly as by stop_tol / stop_patience -- further
 *   steps leave the parameters untouched, gpe_stop_state reports the optimiser step of that record, gpe_reset_optimizer clears it.
 * gpe_pinn/keeper.py:select restates the rule in fp64 for anyone replaying a monitor log.
 * Lifetime: gpe_bind_monitor on an engine with an armed keeper resets it to "nothing kept" and leaves it armed (the metric is comparable
 * on one point set only); clearing the monitor -- also the drop at a new bind with a precomputed base -- disarms it and frees its
 * buffers.  gpe_set_params, gpe_reset_optimizer (the counters go on: a run that stopped by patience stops again at the next record
 * without improvement), gpe_set_gamma, redraws and binds of points leave it alone.  gpe_step_dp / gpe_run_dp and the three-phase
 * entry points ignore it, as they ignore the monitor. */
enum { GPE_KEEP_NONE = 0, GPE_KEEP_RES_RMS = 1, GPE_KEEP_ENERGY = 2 };   /* the field judged: res_rms, energy (struct gpe_observables) */
/* Arms the keeper (a second call re-arms it from "nothing kept"); GPE_KEEP_NONE disarms it.  Allocates a second parameter vector and a
 * small state block here, never later.  GPE_ERR_INVALID: no monitor bound, an unknown metric, min_delta < 0 or not finite, patience < 0
 * (0: never stop), or an engine with a communicator (gpe_comm_init: every rank's monitor sees its own points, the ranks would keep and
 * stop differently).  A bind that fails leaves the keeper that was there, its kept set included. */
int gpe_bind_keeper(gpe_engine* e, int metric, double min_delta, int64_t patience);
/* synchronise; the kept parameters (caller's layout, as gpe_get_params; n == gpe_param_count), the kept record, records judged / kept /
 * judged since the last one kept, and whether the keeper's patience fired the stop.  Any out pointer may be NULL.  GPE_ERR_STATE: no
 * keeper bound.  With nothing kept yet the counters are filled and a request for h_flat or rec fails with GPE_ERR_INVALID. */
int gpe_keeper_read(gpe_engine* e, float* h_flat, size_t n, struct gpe_observables* rec, int64_t* seen, int64_t* kept, int64_t* since_best,
                    int* stopped);
/* The kept parameters become the engine's parameters (device copy, then as gpe_set_params: the packed weight copies are rebuilt
 * before their next use).  Adam moments, scheduler state and the stop flag stay as they are.  GPE_ERR_INVALID: nothing kept yet. */
int gpe_keeper_restore(gpe_engine* e);

/* ---- mixture engines: observables, held-out monitor and keeper (replaces tools/accuracy_mixture.py:state; no reference counterpart) ----
 * The entry points above keep refusing a mixture engine (GPE_ERR_STATE): their record has one norm, one mu and reads two outputs as
 * complex psi.  These five are their mixture instances -- same launch chain with a record of its own (csrc/gpe_observe_mix.h), same
 * lifetime rules -- and return GPE_ERR_STATE on an engine that is not a mixture.  gpe_keeper_restore serves both kinds of engine; on a
 * mixture engine gpe_read_monitor with count > 0 and gpe_keeper_read with rec != NULL return GPE_ERR_STATE (the records are of the other type).
 * gpe_mixture_observables: as gpe_observables (d_x == NULL: the bound collocation points, their bound potential and, under
 * gpe_bind_weights, their weights in every sum -- peak_density stays the plain maximum; an explicit set is unweighted).  The couplings
 * and target norms are read at the launch: a gpe_set_mixture between two records shows in the next one. */
int gpe_mixture_observables(gpe_engine* e, const float* d_x, int64_t n, const float* d_V, float dv, struct gpe_mixture_observables* out);
/* Held-out monitor of a mixture engine: gpe_bind_monitor's cadence, ring, graph cutting in gpe_run and validate-then-swap rules, with
 * records of struct gpe_mixture_observables (unweighted).  d_x == NULL or every <= 0 clears it (and disarms the keeper). */
int gpe_mixture_monitor(gpe_engine* e, const float* d_x, int64_t n, const float* d_V, float dv, int64_t every, int32_t capacity);
/* as gpe_read_monitor */
int gpe_mixture_monitor_read(gpe_engine* e, int64_t first, int64_t count, struct gpe_mixture_observables* out, int64_t* available);
/* Keeper of a mixture engine: gpe_bind_keeper's rule, counters, patience stop, refusals (GPE_ERR_INVALID: no monitor bound, an unknown
 * metric, min_delta < 0 or not finite, patience < 0, an engine with a communicator) and lifetime (a re-bind of the monitor restarts an
 * armed keeper from "nothing kept").  The field judged: GPE_KEEP_RES_RMS res_rms_total, GPE_KEEP_ENERGY energy. */
int gpe_mixture_keeper(gpe_engine* e, int metric, double min_delta, int64_t patience);
/* as gpe_keeper_read, with the mixture record */
int gpe_mixture_keeper_read(gpe_engine* e, float* h_flat, size_t n, struct gpe_mixture_observables* rec, int64_t* seen, int64_t* kept,
                            int64_t* since_best, int* stopped);

/* ---- training step: the epoch body refine/...:328-361 ; nb c10:L84-103 ------------------------------ */
/* phase 1: forward jets + local sums  -> exchange buffer "sums" */
int gpe_step_begin(gpe_engine* e);
/* phase 2: residual, seeds, reverse pass -> exchange buffer "grad" (flat gradient + tail scalars) */
int gpe_step_backward(gpe_engine* e);
/* phase 3: clip_grad_norm_, Adam, scheduler.step(loss), history record */
int gpe_step_update(gpe_engine* e);
/* device buffers to all-reduce(sum) between the phases when world_size > 1 */
int gpe_exchange_sums(gpe_engine* e, void** d_ptr /* double* */, int64_t* count);
int gpe_exchange_grad(gpe_engine* e, void** d_ptr /* float*  */, int64_t* count);
/* Optional: make the engine use CALLER-owned device memory for the two exchange buffers, so that they can be
 * handed to a collective library as that library's own tensor type.  d_dbl: >= gpe_exchange_dbl_count() doubles
 * (the first `count` of gpe_exchange_sums() are the all-reduced part), d_grad: >= P + 4 floats. */
int64_t gpe_exchange_dbl_count(void);
int gpe_use_external_exchange(gpe_engine* e, void* d_dbl, int64_t n_dbl, void* d_grad, int64_t n_grad);
/* ---- data-parallel exchange INSIDE the engine: RCCL over xGMI on a dedicated HIP stream ------------------------------------
 * The reference is single-device (refine/...:12); this is the build's row (e) of SURVEY 8.  One process per GPU:
 *   rank 0: gpe_comm_unique_id() -> 128 bytes, handed to the other ranks by any out-of-band channel (a torch.distributed
 *   store, MPI, a file); every rank: gpe_comm_init(id, rank, world) with gpe_config.world_size == world.
 * gpe_step_dp = gpe_step_begin, ncclAllReduce of the 12 double sums, gpe_step_backward with the gradient all-reduced on the
 * exchange stream (generic kernel set: one bucket per linear map, output map first, overlapped with the rest of the reverse
 * pass; fused set: one P+4 message), gpe_step_update.  Nothing synchronises with the host. */
#define GPE_COMM_ID_BYTES 128
int gpe_comm_unique_id(gpe_engine* e, void* out128);
int gpe_comm_init(gpe_engine* e, const void* id128, int rank, int world);
int gpe_comm_destroy(gpe_engine* e);
int gpe_comm_info(const gpe_engine* e, int* rank, int* world, int64_t* collectives);   /* rank -1 / world 0: no communicator */
int gpe_step_dp(gpe_engine* e);
int gpe_run_dp(gpe_engine* e, int64_t n_steps);
/* OPT-IN one-step-stale gradient: the all-reduce of step t's gradient stays in flight on the exchange stream behind the forward
 * of step t+1; the update of step t applies the (all-reduced) gradient and scalars of step t-1, step 0 applies nothing, records lag
 * one step.  It changes the optimisation trajectory -- not comparable bit for bit with the reference -- and is never enabled
 * implicitly; a run that uses it must say so. */
int gpe_comm_set_async(gpe_engine* e, int on);
/* all three phases + synchronise + scalars (single rank) */
int gpe_step(gpe_engine* e, gpe_scalars* out);
/* n steps enqueued back to back, no host synchronisation (single rank) */
int gpe_run(gpe_engine* e, int64_t n_steps);
/* synchronise and read the scalars of the most recent step / of steps [first, first+count) (1-based) */
int gpe_read_scalars(gpe_engine* e, gpe_scalars* out);
int gpe_read_history(gpe_engine* e, int64_t first_step, int64_t count, gpe_scalars* out);
int gpe_synchronize(gpe_engine* e);
/* early-stop state: *stopped = 1 once a stop condition fired; *stop_step = the optimiser step that fired it (1-based) */
int gpe_stop_state(gpe_engine* e, int* stopped, int64_t* stop_step);

/* ---- pre-training on an analytic target: pretrain_on_analytical_solution (refine/...:650-701) ------------------------
 * loss = mean((NN(x) - target)^2) on the bound points; d_target [n_local,out].  gpe_mse_step: one plain Adam step (no
 * clipping, no scheduler, refine/...:663-670); gpe_mse_loss_grad: loss + gradient without update (the reference's L-BFGS
 * tail, refine/...:672-687, runs host-side on these; read the gradient with gpe_get_grad).  Single-rank entry points; the
 * phases gpe_mse_begin / gpe_mse_update bracket an all-reduce of the gradient exchange buffer when world_size > 1.
 * The pre-training loss is and stays UNWEIGHTED: quadrature weights bound by gpe_bind_weights change neither its sum nor its mean
 * (n_global, or the bound count). */
int gpe_bind_target(gpe_engine* e, const float* d_target);
int gpe_mse_begin(gpe_engine* e);                    /* forward, seeds, reverse -> gradient exchange buffer (tail: sum of squares) */
int gpe_mse_update(gpe_engine* e);                   /* Adam on the exchanged gradient */
int gpe_mse_step(gpe_engine* e, gpe_scalars* out);   /* begin + update + synchronise; out->loss = the MSE */
int gpe_mse_loss_grad(gpe_engine* e, double* loss);

/* ---- device-resident L-BFGS: torch.optim.LBFGS without a line search (the tail of pretrain_on_analytical_solution, refine/...:672-687,
 * and of the 2D hybrid driver), with no host round trip per evaluation.  Without a line search torch's outer / inner loop is the flat
 * sequence "evaluate loss and gradient, iterate": `max_iter` and `tolerance_change` only end an outer call, and the next call
 * re-evaluates at the same parameters and carries on.  One iteration here is that pair: the evaluation's launches, then
 *   y = g - g_prev, s = t d;  the pair is pushed only if y.s > 1e-10 (the oldest leaves at `history`), H = y.s / y.y;
 *   d = -g, t = min(1, 1/|g|_1) lr on the first iteration; afterwards d = -H_k g by the two-loop recursion, t = lr;
 *   no parameter update (everything else proceeds) if g.d > -tolerance_change;  theta += t d otherwise.
 * The state FREEZES for good -- no byte of the parameters or of the L-BFGS state changes any more -- once max|g| <= tolerance_grad,
 * the loss or the gradient is not finite, or loss < stop_loss (0: never).  The loss is the one the Adam update records: the physics
 * total, or the MSE in pre-training mode.  Rings and directions are fp32, every reduction and the recursion fp64; results are the same
 * bits from run to run.  Adam's moments, step count, schedulers and history are neither read nor written.
 * gpe_lbfgs_config: allocates (first call, or a new `history`) and resets the L-BFGS state.  GPE_ERR_INVALID: history outside [1, 128],
 *   lr not finite or <= 0, a tolerance or stop_loss negative or not finite, a data-parallel engine (world_size > 1 or a communicator).
 * gpe_lbfgs_update: the third phase behind gpe_step_backward or gpe_mse_begin, in place of gpe_step_update / gpe_mse_update; reads the
 *   gradient exchange buffer and its tail exactly as those do.
 * gpe_lbfgs_run: n_iters iterations (evaluations, with a line search on: see gpe_lbfgs_line_search) (mse != 0: of the pre-training loss, which needs gpe_bind_target) enqueued back to back with plain
 *   launches; no host synchronisation, no graph capture.  The held-out monitor and the keeper are served by it once gpe_lbfgs_monitor
 *   says so, and then see the JUDGED POINT only: the parameters as they stand without a line search and in every frozen state, the start
 *   point of the running search (the last accepted point) under strong Wolfe -- never a trial point.
 * gpe_lbfgs_read: synchronise; out = (loss, max|g|, |g|_1, t, g.d, n_iter, pairs held, frozen (0 no, 1 tolerance_grad, 2 non-finite,
 *   3 stop_loss, 4 the keeper's patience: gpe_lbfgs_monitor), skipped, pushed, y.s, H_diag, ring head, prev_loss, 0, 0): loss, the gradient norms, g.d, skipped, pushed and y.s are
 *   the last iteration's, the rest the state as it stands.
 * gpe_lbfgs_history: synchronise; the pairs held, oldest first, as rows of h_S / h_Y [history][n], g_prev and d [n], in the caller's
 *   parameter layout (n = gpe_param_count); any pointer may be NULL.
 * gpe_reset_optimizer, gpe_set_params and gpe_keeper_restore reset the L-BFGS state (the configuration stays).
 * GPE_ERR_STATE (update, run): not configured; a sampler with every > 0 bound (the objective would change under the history);
 * gpe_comm_init done.  (read, history): not configured. */
int gpe_lbfgs_config(gpe_engine* e, double lr, int history, double tolerance_grad, double tolerance_change, double stop_loss);
int gpe_lbfgs_update(gpe_engine* e);
int gpe_lbfgs_run(gpe_engine* e, int64_t n_iters, int mse);
int gpe_lbfgs_read(gpe_engine* e, double out[16]);
int gpe_lbfgs_history(gpe_engine* e, float* h_S, float* h_Y, float* h_g_prev, float* h_d, size_t n, int* count);

/* ---- strong-Wolfe line search for the device-resident L-BFGS: torch.optim.LBFGS(line_search_fn="strong_wolfe"), flattened.  With it the
 * flat sequence is "evaluate, TICK": a tick is a line-search decision on the evaluation at the trial point theta0 + t d (torch's
 * `_strong_wolfe` in its order of tests: sufficient decrease / not below the previous trial, curvature, g.d >= 0; extrapolation by cubic
 * interpolation within (t + 0.01 (t - t_prev), 10 t); at max_ls the bracket [0, t]; the zoom loop with its bracket-width break against
 * tolerance_change / max|d|, the 10 % rule and the low / high updates), followed by the L-BFGS iteration ONLY if the decision accepts a
 * point.  The accepted point is the bracket's low end with the loss and gradient STORED for it -- not necessarily the last one evaluated
 * -- and the iteration runs on those; no evaluation is spent on it.  Every tick is the same launch sequence; the host never reads a
 * decision and nothing synchronises.  Rules beyond torch's: the freezes of gpe_lbfgs_config apply at accepted points; a non-finite loss or
 * gradient at a TRIAL puts the parameters back to the best point the bracket holds (its low end, or the start point before a bracket
 * exists) and freezes with code 2, so a frozen run never leaves the parameters at a trial point; `stalled` counts accepted steps with
 * t = 0 (parameters unchanged, no pair pushed) and is not a stop: the evaluation budget bounds the run.
 * gpe_lbfgs_line_search: kind 0 = none (the machine of gpe_lbfgs_update as it is without this call, the same bits), 1 = strong Wolfe.
 *   Needs gpe_lbfgs_config first; allocates on first use (the start point and three trial-gradient slots) and resets the L-BFGS state.
 *   The choice stays across later gpe_lbfgs_config calls.  GPE_ERR_INVALID: unknown kind, c1 or c2 not finite or not 0 < c1 < c2 < 1,
 *   max_ls outside [1, 64].  GPE_ERR_STATE: L-BFGS not configured.
 * With a line search on, gpe_lbfgs_update is ONE TICK and gpe_lbfgs_run's n_iters counts EVALUATIONS (ticks), not iterations.
 *   gpe_lbfgs_read / gpe_lbfgs_history keep their layout and report the last completed iteration: t is then the first trial step of the
 *   new direction, loss the accepted loss, g_prev the gradient at the search's start point.
 * gpe_lbfgs_ls_read: synchronise; out = (phase: what the last tick did, 0 nothing yet, 1 bracket phase went on, 2 zoom went on, 3 a point
 *   was accepted, 4 frozen; ls_iter; evaluations in this search; evaluations in all; t of the next trial; t_prev; bracket ends (2), their
 *   losses (2) and g.d (2) -- after an accepted tick end 0 is the new start point and end 1 the point the search just ended accepted: its
 *   step, loss and g.d along the old direction --; low_pos; loss and g.d at the start point; max|d|; searches accepted; ended by max_ls; by the width break; by
 *   the curvature test; stalled; insuf_progress; the ends' gradient slots (end 0 + 4 * end 1; 3 = the start gradient); the slot of the
 *   next gradient).
 * Every reset of the L-BFGS state ends a running search.  gpe_reset_optimizer and gpe_lbfgs_line_search do not rewrite the parameters:
 *   they put them back to the search's start point first.  gpe_set_params and gpe_keeper_restore overwrite them; a new gpe_lbfgs_config
 *   starts from the parameters as they stand.  The refusals of gpe_lbfgs_update / gpe_lbfgs_run are unchanged. */
int gpe_lbfgs_line_search(gpe_engine* e, int kind, double c1, double c2, int max_ls);
int gpe_lbfgs_ls_read(gpe_engine* e, double out[24]);

/* ---- L-BFGS under the held-out monitor and the keeper (opt-in; off, gpe_lbfgs_run is what it is without these two calls, the same
 * launches and the same bits).  The JUDGED POINT is the one parameter set an observer of an L-BFGS run may look at:
 *   no line search: the parameters as they stand after the tick;  strong Wolfe, search running: the search's start point -- the last
 *   accepted point, or the parameters the run started from (after an accepting tick the parameters are already the first trial of the
 *   next direction);  search idle, or frozen with any code: the parameters as they stand (a frozen run never sits at a trial point).
 * The state that decides this lives on the device and the choice is made there (csrc/gpe_lbfgs.h: k_lbfgs_view, k_lbfgs_unview).
 * gpe_lbfgs_monitor: on = 1: every tick of gpe_lbfgs_run (one evaluation, with or without a line search, mse or not) counts as one step
 *   of the bound monitor's `every`, on the counter gpe_run uses, so an Adam run followed by an L-BFGS tail keeps one rhythm.  On a monitor
 *   tick the judged point takes the parameters' place, the monitor's chain runs as behind an Adam step (record into the ring; with a
 *   keeper: judged, and the judged point copied aside if it is the best), and the parameters come back: the run goes on from the bits it
 *   would have had.  Nothing synchronises.  The record's `step` is what the chain writes: the Adam step count, which L-BFGS does not
 *   advance.  When the keeper's patience fires the run FREEZES for good with code 4: the parameters stay at the judged point of that
 *   record, a running search is ended, gpe_stop_state reports the stop as after gpe_run.  What clears it is what resets the L-BFGS
 *   state and the stop (gpe_reset_optimizer); re-arm the keeper to start a new count.  Records go on being written after any freeze, of
 *   the parameters as they stand.  on = 0 (the default): ticks do not count.  With no monitor bound the flag does nothing.  It stays
 *   across gpe_lbfgs_config and gpe_lbfgs_line_search calls; gpe_lbfgs_update alone ignores the monitor, as the three-phase entry
 *   points do.  Allocates one parameter vector at the first on = 1.  GPE_ERR_INVALID: on is not 0 or 1.  GPE_ERR_STATE: L-BFGS not
 *   configured.
 * gpe_lbfgs_point: synchronise; the judged point in the caller's parameter layout (n = gpe_param_count).  Writes nothing on the device:
 *   a running search goes on from the same bits.  GPE_ERR_INVALID: h_flat NULL or a wrong n.  GPE_ERR_STATE: L-BFGS not configured. */
int gpe_lbfgs_monitor(gpe_engine* e, int on);
int gpe_lbfgs_point(gpe_engine* e, float* h_flat, size_t n);

/* ---- continuation knobs: the gamma / perturbation loop of refine/...:289-340 -------------------------- */
int gpe_set_gamma(gpe_engine* e, float gamma);
/* mixture engines: the coupling matrix (g_11, g_22, g_12) of the NEXT step (gamma-continuation), like gpe_set_gamma: takes effect at the
 * next enqueued step, a captured graph is rebuilt.  GPE_ERR_STATE: not a mixture engine; GPE_ERR_INVALID: a non-finite coupling. */
int gpe_set_mixture(gpe_engine* e, float g11, float g22, float g12);
/* synchronise; out = (mu_1, mu_2, I_1, I_2, num_1, den_1, num_2, den_2) of the last completed step or gpe_residual (the numbers its
 * gpe_scalars record was formed from; over all ranks in a data-parallel step).  GPE_ERR_STATE: not a mixture engine. */
int gpe_mixture_scalars(gpe_engine* e, double out[8]);
/* mixture engines: the energy term.  With q the quadrature weights (1 without), den_a = sum q u_a^2, I_a = dx den_a,
 *   T_a = sum q (c |grad u_a|^2 + V u_a^2),   Q_ab = sum q u_a^2 u_b^2,
 * the energy of the state normalised to the target norms, v_a = u_a sqrt(n_a / I_a), is
 *   E = sum_a n_a T_a / den_a + 1/2 sum_ab g_ab n_a n_b Q_ab / (den_a den_b dx)            (g_21 = g_12: the 12 term counts twice)
 *   loss += w_E E
 * E does not change when a component is scaled; its stationary points under the two norm constraints are the solutions of
 * H_a v_a = mu_a v_a and its minimiser is the ground state (at g_12 = 0, n = (1, 1) it is the sum of two GPE_RIESZ_VARIATIONAL energies
 * at p = 3).  Seeds at the output jets (times q_i and perturb_scale as all seeds), with alpha_a = n_a / den_a,
 * beta_aa = 1/2 g_aa n_a^2 / (den_a^2 dx), beta_12 = g_12 n_1 n_2 / (den_1 den_2 dx), b the other component:
 *   delta_a    = -n_a T_a / den_a^2 - g_aa n_a^2 Q_aa / (den_a^3 dx) - g_12 n_1 n_2 Q_12 / (den_a^2 den_b dx)
 *   d/du_a     = w_E (2 alpha_a V u_a + 4 beta_aa u_a^3 + 2 beta_12 u_a u_b^2 + 2 delta_a u_a)
 *   d/d(d_k u_a) = w_E 2 c alpha_a d_k u_a ;   d/d(lap u_a) unchanged
 * The five sums travel in slots 2-6 of the first exchange message, which a mixture engine leaves empty otherwise; the coefficients are
 * formed in double from the all-reduced sums.
 * gpe_mixture_energy_weight: w_E of the NEXT step, like gpe_set_mixture (a captured graph is rebuilt); a step with w_E != 0 runs the
 * energy instances of the head and seed kernels, adds w_E E to the loss and reports E in gpe_scalars.riesz; w_E = 0 (the default) is the
 * plain mixture step, kernel for kernel.  GPE_ERR_STATE: not a mixture engine; GPE_ERR_INVALID: a negative or non-finite weight.
 * gpe_mixture_energy: forward-only evaluation on the bound set at the current parameters, at any w_E (0 included); synchronises;
 * out = (E, T_1, T_2, Q_11, Q_22, Q_12, den_1, den_2), over all ranks when a communicator is up (every rank calls it).  Parameters,
 * optimiser state and the last record are left as they were.  GPE_ERR_STATE: not a mixture engine, or nothing bound. */
int gpe_mixture_energy_weight(gpe_engine* e, float w_E);
int gpe_mixture_energy(gpe_engine* e, double out[8]);
int gpe_set_power(gpe_engine* e, int p);
int gpe_set_lr(gpe_engine* e, float lr);
int gpe_set_perturb_scale(gpe_engine* e, float s);
int gpe_set_n_global(gpe_engine* e, int64_t n_global);   /* GPE_ERR_STATE while quadrature weights are bound: N is their total W */
/* loss weights between steps: the host-side ReLoBRaLo balancing of src/gross_pitaevskii_2D_ReLoBRaLo.py:259-342 only needs the
 * per-term scalars gpe_residual / gpe_step return and this setter.  w[6] = {pde, bc, norm, sym, orth, riesz}. */
int gpe_set_loss_weights(gpe_engine* e, const float w[6]);

/* Per-kernel timing with HIP events on the engine's stream (for bench.py's roofline object).  While enabled, every
 * launch of the two dominant kernels on the collocation batch (jet forward, jet reverse) is bracketed by events.
 * gpe_profile_read synchronises and returns out[0]=forward ms total, out[1]=forward launches, out[2]=reverse ms total,
 * out[3]=reverse launches (since the last enable), then clears the counters. */
int gpe_profile_enable(gpe_engine* e, int on);
int gpe_profile_read(gpe_engine* e, double out[4]);

/* bytes of HBM traffic one step is designed to move (B_mat-style accounting, for bench.py) and FLOPs */
int gpe_step_cost(const gpe_engine* e, double* flops_per_point, double* hbm_bytes_per_point);

#ifdef __cplusplus
}
#endif
#endif /* GPE_HIP_H */
