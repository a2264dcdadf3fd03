// gpe_update.h -- the update kernels: grad-norm clip, Adam, LR scheduler, history record, and the slab reductions that hand over to them.
// Included by gpe_engine.hip behind the kernel headers it builds on (gpe_common.h, gpe_head.h, gpe_observe_mix.h, gpe_fused.h).
#pragma once
#define UPD_REG_E 13            // elements per thread the single-workgroup update keeps in registers (update_core; the host mirrors the bound)
// ------------------------------------------------------------------------------------------------
// update kernel: clip_grad_norm_ + Adam + scheduler + record   (refine/...:359-361, 364-381)
// ------------------------------------------------------------------------------------------------
// Large parameter vectors (P >= UPD_MULTI_MIN: [2,128x5,1] and up) run the update on UPD_G workgroups -- one workgroup took 0.40 ms
// per step at P = 330 241.  k_update_part: per-workgroup partial sums of |g|^2 over contiguous chunks (fixed order: deterministic
// for a given P) + a snapshot of the step sums and of the optimiser state; k_update<true>: every workgroup adds the partial sums in the
// same order and derives the same clip factor / step size from the SNAPSHOTS (workgroup 0 alone writes the optimiser state, the
// record and the history, and zeroes the step sums), then updates its chunk.  The repacking of the hidden-hidden weights needs ALL
// updated parameters, so it is left to the next step's k_begin in this mode.
#define UPD_G 64
#define UPD_MULTI_MIN 32768
struct UpdSnap { double sums[S_COUNT]; double lsums[LS_COUNT]; OptDev od; double part[UPD_G]; };
GPE_DEV int upd_chunk(int P) { return (((P + UPD_G - 1) / UPD_G) + 3) & ~3; }
static int upd_chunk_host(int P) { return (((P + UPD_G - 1) / UPD_G) + 3) & ~3; }
__global__ __launch_bounds__(1024) void k_update_part(int P, const float* __restrict__ grad, const double* __restrict__ sums,
                                                       const double* __restrict__ lsums, const OptDev* __restrict__ od,
                                                       UpdSnap* __restrict__ snap) {
    __shared__ double red[16];
    const int chunk = upd_chunk(P), lo = blockIdx.x * chunk, hi = min(P, lo + chunk);
    double acc = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += 1024) { double g = grad[i]; acc += g * g; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < 16; ++i) tot += red[i];
        snap->part[blockIdx.x] = tot;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < S_COUNT) snap->sums[threadIdx.x] = sums[threadIdx.x];
        if (threadIdx.x < LS_COUNT) snap->lsums[threadIdx.x] = lsums[threadIdx.x];
        if (threadIdx.x == 64) snap->od = *od;
    }
}

// one Adam element, torch's op order (refine/...:359-361): shared by every update loop so that they agree bit for bit
GPE_DEV void adam_element(float graw, float& m, float& v, float& th, float coef, float ss, float b2s, float b1, float b2, float eps) {
#pragma clang fp contract(off)      // torch's kernels round every product before the add; and every call site must round alike
    const float g = graw * coef;
    m = m + (g - m) * (1.0f - b1);                 // exp_avg.lerp_(grad, 1-beta1)
    v = v * b2 + (1.0f - b2) * g * g;              // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1-beta2)
    const float denom = sqrtf(v) / b2s + eps;
    th = th - ss * (m / denom);                    // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// gradient element as the update reads it.  SC1 (the update runs inside the slab-reduction launch, k_reduce_update below): the values
// were stored by OTHER workgroups of this launch with write-through (sc1) stores -- read them past this CU's L1
template <bool SC1>
GPE_DEV float grad_load(const float* p) {
    if constexpr (SC1) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

// W_j[n][kk] of a hidden-hidden map -> its slots in the two packed copies (pack_weight_element inverted): the update SCATTERS the new
// weights instead of a gather pass behind a barrier
GPE_DEV void scatter_pack(const NetDesc& nd, int H, int i, float th, float* __restrict__ Wpk, float* __restrict__ WpkT) {
    const int lg = H == 64 ? 6 : (H == 32 ? 5 : (H == 128 ? 7 : 8)), NT = H >> 4, maps = nd.n_lin - 2;
    for (int j = 1; j <= maps; ++j) {
        const int e = i - nd.offW[j];
        if (e >= 0 && e < H * H) {
            const int n = e >> lg, kk = e & (H - 1);
            const int nt = n >> 4, kt = kk >> 4;
            Wpk[(((j - 1) * NT + nt) * NT + kt) * 256 + ((n & 15) + 16 * ((kk & 15) >> 2)) * 4 + (kk & 3)] = th;
            WpkT[(((j - 1) * NT + kt) * NT + nt) * 256 + ((kk & 15) + 16 * ((n & 15) >> 2)) * 4 + (n & 3)] = th;
        }
    }
}

template <bool MULTI, bool SC1 = false>
GPE_DEV void update_core(int P, float* __restrict__ theta, float* __restrict__ am,
                         float* __restrict__ av, const float* __restrict__ grad,
                         const double* __restrict__ sums_in, const double* __restrict__ lsums_in,
                         const Phys& ph, const OptCfg& oc, OptDev* __restrict__ od,
                         gpe_scalars* __restrict__ hist, int cap, gpe_scalars* __restrict__ last,
                         double bc_cnt, int do_update, int mse_mode, const NetDesc& nd, int H,
                         float* __restrict__ Wpk, float* __restrict__ WpkT, int n_pack,
                         double* __restrict__ dbl, int n_dbl, double* __restrict__ dbl_keep,
                         const UpdSnap* __restrict__ snap, int pack_mode) {
    // pack_mode (one workgroup): 1 = repack the hidden-hidden weights by a gather pass over the updated parameters (also writes the
    // bf16 pieces the opt-in split-bf16 kernels read); 2 = every thread SCATTERS its updated weights into the two packed copies inside
    // the Adam loop (no second pass, no barrier, no bf16 pieces).  REG_E: up to this many elements per thread are loaded ONCE, at the
    // top, into registers (gradient for the norm, Adam moments and parameters behind it): at the reference's batch sizes this kernel
    // is a chain of dependent round trips to L2 -- it took 16.6 us of a 52 us step at 4 000 points -- and every load issued early is
    // one round trip less.
    constexpr int REG_E = UPD_REG_E;                               // (13 312 parameters: the 4 x 64 networks of BASELINE; 16 would spill at 128 registers)
    const bool cached = !MULTI && P <= REG_E * 1024 && !(pack_mode & 4);      // (bit 2 of pack_mode: tuning switch GPE_UPDATE_CACHE=0)
    pack_mode &= 3;
    float cg[REG_E], cm[REG_E], cv[REG_E], ct[REG_E];
    __shared__ double red[16];
    __shared__ float s_coef, s_ss, s_b2s;
    __shared__ int s_skip, s_book, s_frozen;
    __shared__ long long s_step;
    __shared__ gpe_scalars s_rec;
    const double* sums = MULTI ? snap->sums : sums_in;
    const double* lsums = MULTI ? snap->lsums : lsums_in;
    const OptDev* odr = MULTI ? &snap->od : od;                    // state the step size is derived from
    const bool lead = !MULTI || blockIdx.x == 0;                   // the workgroup that writes the optimiser state / record / history
    const int lo = MULTI ? blockIdx.x * upd_chunk(P) : 0, hi = MULTI ? min(P, lo + upd_chunk(P)) : P;
    // the scalars thread 0 needs behind the norm are requested NOW, beside the elements: one round trip less in its serial section
    double p_num = 0.0, p_den = 0.0, p_bcse = 0.0, p_lr = 0.0, p_b1p = 0.0, p_b2p = 0.0;
    float p_sr2 = 0.f;
    long long p_step = 0;
    int p_stopped = 0;
    if (threadIdx.x == 0) {
        p_num = sums[S_NUM]; p_den = sums[S_DEN]; p_bcse = lsums[LS_BC_SE2]; p_sr2 = grad_load<SC1>(&grad[P + GT_SUM_R2]);
        p_lr = odr->lr; p_b1p = odr->b1p; p_b2p = odr->b2p; p_step = odr->step; p_stopped = odr->stopped;
    }
    // mixture energy term: in the single-workgroup forms E is formed by the first thread of wave 1 ahead of the barrier below -- inside thread
    // 0's serial section, the kernel's register peak, it cost four more spilled VGPRs and 0.7 % of the headline step
    const bool mix_en = oc.mix.on && oc.mix.wE != 0.f;
    __shared__ double s_mixE;
    if constexpr (!MULTI) {
        if (mix_en && threadIdx.x == 64) s_mixE = mix_energy_of(oc.mix.g, oc.mix.n, (double)ph.dx, sums).E;
        double acc = 0.0;
        if (cached) {
#pragma unroll
            for (int k = 0; k < REG_E; ++k) { const int i = threadIdx.x + k * 1024; cg[k] = i < P ? grad_load<SC1>(&grad[i]) : 0.f; }
#pragma unroll
            for (int k = 0; k < REG_E; ++k) {
                const int i = threadIdx.x + k * 1024;
                if (i < P) { cm[k] = am[i]; cv[k] = av[i]; ct[k] = theta[i]; }
            }
#pragma unroll
            for (int k = 0; k < REG_E; ++k) { const double g = cg[k]; acc += g * g; }          // (same order as the loop below)
        } else
        for (int i = threadIdx.x; i < P; i += 1024) { double g = grad_load<SC1>(&grad[i]); acc += g * g; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double tot = 0.0;
        if constexpr (MULTI) { for (int i = 0; i < UPD_G; ++i) tot += snap->part[i]; }
        else { for (int i = 0; i < 16; ++i) tot += red[i]; }
        double gn = sqrt(tot);
        double num = p_num, den = p_den;
        double lam = (double)(float)lambda_of(ph, sums, num, den);
        double I = (double)((float)den * ph.dx);
        double sr2 = (double)p_sr2;
        double pde = sr2 / ph.n_global;
        double nrm = (I - 1.0) * (I - 1.0);
        if (oc.mix.on) {                  // two real components: one Rayleigh quotient and one norm term each; the record carries component 1
            const double num2 = sums[S_MIX_NUM2], den2 = sums[S_MIX_DEN2];
            const double lam2 = (double)(float)(num2 / den2), I2 = (double)((float)den2 * ph.dx);
            lam = (double)(float)(num / den);
            const double d1 = I - (double)oc.mix.n[0], d2 = I2 - (double)oc.mix.n[1];
            nrm = d1 * d1 + d2 * d2;
            if (lead && !mse_mode && !(do_update && p_stopped)) {
                od->mix[0] = lam; od->mix[1] = lam2; od->mix[2] = I; od->mix[3] = I2;
                od->mix[4] = num; od->mix[5] = den; od->mix[6] = num2; od->mix[7] = den2;
            }
        }
        double bc = bc_cnt > 0 ? p_bcse / bc_cnt : 0.0;
        double sym = ph.w_sym != 0.f ? sums[S_SYM] / ph.n_global : 0.0;
        double orth = 0.0;
        for (int j = 0; j < ph.n_orth; ++j) { double oj = sums[S_ORTH0 + j] * ph.dx; orth += oj * oj; }
        double riesz = 0.0;
        if (ph.w_riesz != 0.f) {          // (the sums are also filed for the energy-functional lambda; the TERM only with its weight)
            const double fI = ph.riesz_kind == GPE_RIESZ_VARIATIONAL ? pow(I, -0.5 * (double)(ph.p - 1)) : 1.0;
            const double Lrot = ph.complex_psi ? (double)ph.omega_rot * sums[S_RZ_L] : 0.0;      // rotating frame: - Omega <L_z>
            riesz = (sums[S_RZ_K] + sums[S_RZ_P] + fI * sums[S_RZ_I] - Lrot) / (ph.riesz_kind == GPE_RIESZ_SUM ? 1.0 : den);
        }
        double reg = reg_terms(ph, den, lam);
        double loss = ph.w_pde * pde + ph.w_bc * bc + ph.w_norm * nrm + ph.w_sym * sym + ph.w_orth * orth + ph.w_riesz * riesz + reg;
        if (mix_en) {        // mixture energy term: E of the state normalised to the target norms, reported as riesz
            if constexpr (MULTI) riesz = mix_energy_of(oc.mix.g, oc.mix.n, (double)ph.dx, sums).E;
            else riesz = s_mixE;
            loss += (double)oc.mix.wE * riesz;
        }
        if (mse_mode) {           // pre-training: loss = mean((NN - target)^2); plain Adam (no clip, no scheduler, no early stop)
            loss = (double)grad_load<SC1>(&grad[P + GT_MSE_SE2]) / (ph.n_global * ph.n_out);
            lam = 0.0; pde = 0.0; nrm = 0.0; bc = 0.0; sym = 0.0; orth = 0.0; riesz = 0.0; reg = 0.0;
        }
        int skip = !(isfinite(loss) && isfinite(gn));
        const int frozen = do_update && p_stopped;
        long long step = p_step + (do_update && !skip && !frozen ? 1 : 0);
        double lr = p_lr;
        float coef = 1.0f;
        if (oc.clip_norm > 0.f && !mse_mode) coef = (float)fmin(1.0, (double)oc.clip_norm / (gn + 1e-6));
        const bool commit = do_update && !skip && !frozen;
        const double b1p = commit ? p_b1p * (double)oc.beta1 : p_b1p, b2p = commit ? p_b2p * (double)oc.beta2 : p_b2p;
        if (commit && lead) { od->b1p = b1p; od->b2p = b2p; }
        double bc1 = 1.0 - b1p;
        double bc2 = 1.0 - b2p;
        s_coef = coef;
        s_ss = (float)(lr / bc1);
        s_b2s = (float)sqrt(bc2);
        s_skip = skip || !do_update || frozen;
        gpe_scalars r;
        r.loss = loss; r.pde = pde; r.bc = bc; r.norm = nrm; r.sym = sym; r.orth = orth; r.mu = lam;
        r.num = num; r.den = den; r.sum_r2 = sr2; r.integral = I; r.grad_norm = gn; r.lr = lr;
        r.step = (double)step; r.nonfinite = skip ? 1.0 : 0.0; r.riesz = riesz; r.reg = reg;
        s_rec = r; s_step = step; s_frozen = frozen; s_book = 1;
    }
    __syncthreads();
    // bookkeeping (record, history, early stop, scheduler: double-precision log / pow / cos) on the last thread, concurrently
    // with the Adam loop of the others
    if (threadIdx.x == 1023 && s_book && lead) {
        const gpe_scalars r = s_rec;
        const long long step = s_step;
        const int frozen = s_frozen, skip = r.nonfinite != 0.0;
        const double loss = r.loss;
        if (!frozen) *last = r;
        if (do_update && !frozen) {
            if (!skip) {
                hist[(step - 1) % cap] = r;
                od->step = step;
                if (mse_mode) { /* no scheduler / early-stop bookkeeping while pre-training */ }
                else {
                // early stopping bookkeeping (refine/...:366-372, 389-400)
                if (loss < od->es_best) { od->es_best = loss; od->es_count = 0; } else od->es_count += 1;
                if ((oc.stop_tol > 0.f && loss <= (double)oc.stop_tol) ||
                    (oc.stop_patience > 0 && od->es_count >= oc.stop_patience)) { od->stopped = 1; od->stop_step = step; }
                // scheduler.step(total_loss)
                if (oc.sched == GPE_SCHED_COSINE_LOSS) {           // quirk Q4: the loss value is the epoch
                    double epoch = (double)(float)loss, T_cur, T_i;
                    if (epoch >= oc.T_0) {
                        if (oc.T_mult == 1.0f) { T_cur = fmod(epoch, (double)oc.T_0); T_i = oc.T_0; }
                        else {
                            int n = (int)(log(epoch / oc.T_0 * (oc.T_mult - 1.0) + 1.0) / log((double)oc.T_mult));
                            T_cur = epoch - oc.T_0 * (pow((double)oc.T_mult, n) - 1.0) / (oc.T_mult - 1.0);
                            T_i = oc.T_0 * pow((double)oc.T_mult, n);
                        }
                    } else { T_i = oc.T_0; T_cur = epoch; }
                    od->lr = oc.eta_min + (od->lr0 - oc.eta_min) * (1.0 + cos(M_PI * T_cur / T_i)) / 2.0;
                } else if (oc.sched == GPE_SCHED_PLATEAU) {        // ReduceLROnPlateau(mode='min', rel threshold)
                    if (loss < od->best * (1.0 - oc.threshold)) { od->best = loss; od->num_bad = 0; }
                    else od->num_bad += 1;
                    if (od->num_bad > oc.patience) {
                        double nl = fmax(od->lr * oc.factor, (double)oc.min_lr);
                        if (od->lr - nl > 1e-8) od->lr = nl;
                        od->num_bad = 0;
                    }
                }
                }
            } else {
                od->nonfinite = 1;
            }
        }
    }
    if (!s_skip && cached) {
        const float coef = s_coef, ss = s_ss, b2s = s_b2s;
        const float b1 = oc.beta1, b2 = oc.beta2, eps = oc.eps;
#pragma unroll
        for (int k = 0; k < REG_E; ++k) {
            const int i = threadIdx.x + k * 1024;
            if (i < P) {
                float m = cm[k], v = cv[k], th = ct[k];
                adam_element(cg[k], m, v, th, coef, ss, b2s, b1, b2, eps);
                theta[i] = th;
                am[i] = m; av[i] = v;
                if (pack_mode == 2 && n_pack > 0) scatter_pack(nd, H, i, th, Wpk, WpkT);
            }
        }
    } else if (!s_skip) {
        const float coef = s_coef, ss = s_ss, b2s = s_b2s;
        const float b1 = oc.beta1, b2 = oc.beta2, eps = oc.eps;
        for (int i = lo + threadIdx.x; i < hi; i += 1024) {
            float m = am[i], v = av[i], th = theta[i];
            adam_element(grad_load<SC1>(&grad[i]), m, v, th, coef, ss, b2s, b1, b2, eps);
            theta[i] = th;
            am[i] = m; av[i] = v;
            if (MULTI && pack_mode == 2 && n_pack > 0) scatter_pack(nd, H, i, th, Wpk, WpkT);      // (small networks on the split update)
        }
    }
    // Prepare the NEXT step, so that it can start with its forward kernel: the step sums are consumed (thread 0 read them
    // before the barrier above) -> zero them; repack the hidden-hidden weights in MFMA fragment order from the new parameters.
    __syncthreads();
    // (stale-gradient mode: this step's sums are kept for the NEXT update, which applies this step's gradient)
    if (lead) for (int i = threadIdx.x; i < n_dbl; i += 1024) { if (dbl_keep) dbl_keep[i] = dbl[i]; dbl[i] = 0.0; }
    if constexpr (!MULTI) {
        if (pack_mode != 2 || !cached || s_skip)                  // (a skipped update leaves the parameters, and with them the packed copies, as they were -- but a repack is harmless)
            for (int i = threadIdx.x; i < n_pack; i += 1024) pack_weight_element(nd, H, theta, Wpk, WpkT, i);
    }
}

template <bool MULTI>
__global__ __launch_bounds__(1024) void k_update(int P, float* __restrict__ theta, float* __restrict__ am,
                                                  float* __restrict__ av, const float* __restrict__ grad,
                                                  const double* __restrict__ sums_in, const double* __restrict__ lsums_in,
                                                  Phys ph, OptCfg oc, OptDev* __restrict__ od,
                                                  gpe_scalars* __restrict__ hist, int cap, gpe_scalars* __restrict__ last,
                                                  double bc_cnt, int do_update, int mse_mode, NetDesc nd, int H,
                                                  float* __restrict__ Wpk, float* __restrict__ WpkT, int n_pack,
                                                  double* __restrict__ dbl, int n_dbl, double* __restrict__ dbl_keep,
                                                  const UpdSnap* __restrict__ snap, int pack_mode) {
    update_core<MULTI>(P, theta, am, av, grad, sums_in, lsums_in, ph, oc, od, hist, cap, last, bc_cnt, do_update, mse_mode, nd, H,
                       Wpk, WpkT, n_pack, dbl, n_dbl, dbl_keep, snap, pack_mode);
}

// closes the reverse phase: adds the boundary-batch gradient (computed on the side stream) and fills the exchange tail
__global__ void k_tail(float* __restrict__ grad, const float* __restrict__ add, int P, const double* dsc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (add && i < P) grad[i] += add[i];
    if (i == 0) { grad[P + GT_SUM_R2] = (float)dsc[0]; grad[P + GT_MSE_SE2] = (float)dsc[2]; }
}

// Slab reduction AND update in one launch (small parameter vectors, whole steps: gpe_step / gpe_run).  At the reference's batch sizes
// the update was a launch of its own whose ONE workgroup started only when the whole reduction grid had drained: 2.6 us of launch plus a
// chain of dependent L2 round trips (10.4 of a 40.5 us step at 4 000 points).  Here every workgroup reduces its 64 columns as
// k_grad_reduce does and stores them write-through (sc1: no L2 write-back fence -- the release fence in every workgroup is what made the
// round-3 attempt at this fusion slower), takes a ticket, and the workgroup whose ticket is the last runs the single-workgroup update on
// the spot, reading the gradient past its L1 (hand-off form of MI355X_MICROARCH.md, "Valid forms": sc1 stores, every storing wave's
// vmcnt(0), workgroup barrier, one agent-scope atomic add per workgroup, the last adder loads sc1 behind a barrier).  Same arithmetic in
// the same order as k_grad_reduce + k_update<false>: bit-identical results (test_update_kernel_forms_are_bit_identical).
__global__ __launch_bounds__(1024) void k_reduce_update(const float* __restrict__ gslab, int nslab, int Ppad, int P, float* __restrict__ grad,
                                                         const float* __restrict__ add, const double* __restrict__ tail_dsc,
                                                         unsigned* __restrict__ ticket,
                                                         float* __restrict__ theta, float* __restrict__ am, float* __restrict__ av,
                                                         const double* __restrict__ sums_in, const double* __restrict__ lsums_in,
                                                         Phys ph, OptCfg oc, OptDev* __restrict__ od, gpe_scalars* __restrict__ hist, int cap,
                                                         gpe_scalars* __restrict__ last, double bc_cnt, NetDesc nd, int H,
                                                         float* __restrict__ Wpk, float* __restrict__ WpkT, int n_pack,
                                                         double* __restrict__ dbl, int n_dbl, int pack_mode) {
    __shared__ float red[16][64];
    __shared__ int s_last;
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const float s = i < P ? slab_column_sum(gslab, nslab, Ppad, i, g) : 0.f;
    red[g][lane] = s;
    __syncthreads();
    if (g == 0 && i < P) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][lane];
        if (add) t += add[i];
        __hip_atomic_store(&grad[i], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        __hip_atomic_store(&grad[P + GT_SUM_R2], (float)tail_dsc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&grad[P + GT_MSE_SE2], (float)tail_dsc[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // every storing wave: its stores have left the CU
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == gridDim.x - 1;
        if (s_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // every other workgroup has drawn: ready for the next launch
    }
    __syncthreads();
    if (!s_last) return;
    update_core<false, true>(P, theta, am, av, grad, sums_in, lsums_in, ph, oc, od, hist, cap, last, bc_cnt, 1, 0, nd, H, Wpk, WpkT, n_pack, dbl,
                             n_dbl, nullptr, nullptr, pack_mode);
}

// Slab reduction of SMALL parameter vectors for whole steps (gpe_step / gpe_run), in the partition of the multi-workgroup update: UPD_G
// workgroups, workgroup b owns the parameters [b chunk, (b+1) chunk), chunk = upd_chunk(P) <= 1024.  Besides the gradient it leaves what
// k_update_part would: the partial sums of |g|^2 (fixed order) and the snapshot of the step sums / optimiser state -- so the update that
// follows is k_update<true> on UPD_G workgroups, a handful of elements per thread, instead of ONE workgroup walking all P parameters through
// a chain of dependent L2 round trips (10.4 us of a 40.5 us step at 4 000 points).  Threads: column = t % chunk, slab group = t / chunk.
__global__ __launch_bounds__(1024) void k_grad_reduce_part(const float* __restrict__ gslab, int nslab, int Ppad, int P, float* __restrict__ grad,
                                                            const float* __restrict__ add, const double* __restrict__ tail_dsc,
                                                            const double* __restrict__ sums, const double* __restrict__ lsums,
                                                            const OptDev* __restrict__ od, UpdSnap* __restrict__ snap) {
    __shared__ float red[1024];
    __shared__ double red2[16];
    const int chunk = upd_chunk(P), lo = blockIdx.x * chunk;
    const int ng = 1024 / chunk;                                  // slab groups (>= 1: chunk <= 1024 is checked by the launcher)
    const int col = threadIdx.x % chunk, grp = threadIdx.x / chunk;
    const int i = lo + col;
    float s = 0.f;
    if (grp < ng && i < P) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;            // four loads in flight per thread (fixed order of the final sum)
        int b = grp;
        for (; b + 3 * ng < nslab; b += 4 * ng) {
            s0 += gslab[(size_t)b * Ppad + i];
            s1 += gslab[(size_t)(b + ng) * Ppad + i];
            s2 += gslab[(size_t)(b + 2 * ng) * Ppad + i];
            s3 += gslab[(size_t)(b + 3 * ng) * Ppad + i];
        }
        for (; b < nslab; b += ng) s0 += gslab[(size_t)b * Ppad + i];
        s = (s0 + s1) + (s2 + s3);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    double gsq = 0.0;
    if (grp == 0 && i < P) {
        float t = 0.f;
        for (int k = 0; k < ng; ++k) t += red[k * chunk + col];
        if (add) t += add[i];
        grad[i] = t;
        gsq = (double)t * (double)t;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gsq += __shfl_down(gsq, o, 64);
    if ((threadIdx.x & 63) == 0) red2[threadIdx.x >> 6] = gsq;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int k = 0; k < 16; ++k) tot += red2[k];
        snap->part[blockIdx.x] = tot;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < S_COUNT) snap->sums[threadIdx.x] = sums[threadIdx.x];
        if (threadIdx.x < LS_COUNT) snap->lsums[threadIdx.x] = lsums[threadIdx.x];
        if (threadIdx.x == 64) snap->od = *od;
        if (threadIdx.x == 65) { grad[P + GT_SUM_R2] = (float)tail_dsc[0]; grad[P + GT_MSE_SE2] = (float)tail_dsc[2]; }
    }
}
