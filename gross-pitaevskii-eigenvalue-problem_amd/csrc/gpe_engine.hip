// gpe_engine.hip -- step orchestrator + C ABI (include/gpe_hip.h) of libgpe_hip.so.  gfx950 only.
//
// One engine = one GPU = one stream.  A training step (the epoch body of
// refine/harmonic_pinn_simulation.py:328-361 / nb c10:L84-103) is three phases:
//   begin    : [pack weights] zero accumulators; jet forward on the collocation batch; head (u, Hu, sums)
//              [+ symmetry batch forward]                        -> "sums" exchange buffer (double[8])
//   backward : lambda, residual, seeds; reverse pass; boundary batch fwd+bwd [+ symmetry bwd]
//                                                                 -> "grad" exchange buffer (float[P+4])
//   update   : grad-norm clip, Adam, LR scheduler, history record (one single-workgroup kernel)
// With world_size > 1 the caller all-reduces the two exchange buffers between the phases (RCCL).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

// RCCL is dlopen'ed at gpe_comm_init: no link-time dependency, and no build-time one either -- the handful of types and enum
// values the five entry points need are declared here as rccl.h (NCCL 2.x ABI) declares them.
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
typedef enum { ncclFloat = 7, ncclDouble = 8 } ncclDataType_t;
}

#include "gpe_common.h"
#include "gpe_head.h"
#include "gpe_observe.h"
#include "gpe_observe_mix.h"
#include "gpe_sampler.h"
#include "gpe_sampler_plan.h"
#include "gpe_potential.h"
#include "gpe_generic.h"
#include "gpe_fused.h"
#include "gpe_wide_api.h"
#include "gpe_env.h"
#include "gpe_dispatch.h"
#include "gpe_lbfgs.h"

static thread_local std::string g_create_error;

#define HIPCHK(e, call)                                                                          \
    do {                                                                                         \
        hipError_t _st = (call);                                                                 \
        if (_st != hipSuccess) {                                                                 \
            char _b[512];                                                                        \
            snprintf(_b, sizeof _b, "%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(_st)); \
            (e)->err = _b;                                                                       \
            return GPE_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

#define FAIL(e, code, ...)                                \
    do {                                                  \
        char _b[512];                                     \
        snprintf(_b, sizeof _b, __VA_ARGS__);             \
        (e)->err = _b;                                    \
        return (code);                                    \
    } while (0)

static inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

#include "gpe_update.h"
#define DBL_COUNT (S_COUNT + LS_COUNT + 4)      // doubles of gpe_engine::dbl: [S_COUNT sums | LS_COUNT local | 4 misc]

// ------------------------------------------------------------------------------------------------
struct Batch {
    Pts pts = {nullptr, nullptr, 0};   // point coordinates [n][dim]: rows [0,na) from a, the rest from b (merged boundary points)
    const float* V = nullptr;
    int64_t n = 0, ld = 0;
    int C = 1, E = 0;              // channels: 1 value + D first derivatives + E second-order channels (gpe_common.h)
    float* O = nullptr;            // [C][n_out][ld]
    float* Ob = nullptr;
    float* u = nullptr;            // [n_out][ld]  (main batch)
    float* Hu = nullptr;
    float* ux = nullptr;           // [dim][ld] grad u (Riesz term)
    float* stored = nullptr;       // fused: fragment-native stored activations
    float* Z0 = nullptr;           // wide set: adjoint-jet ping-pong buffers [tile][C][H/16][256]
    float* Z1 = nullptr;
    std::vector<float*> S;         // generic: per hidden layer [C][H][ld]
    float* A0 = nullptr;           // generic adjoint ping/pong [C][maxW][ld]
    float* A1 = nullptr;
    float* A2 = nullptr;           // third adjoint buffer (residual networks: a block's output adjoint waits for the skip join)
    float* xown = nullptr;         // owned copy of points (symmetry batch)
    std::vector<void*> allocs;
};

// the parameter set a forward pass evaluates, with its packed copies (fused path): the trained one, or a frozen orthogonality state's
struct FwdWeights { const float* theta; const float* Wpk; const float* WpkT; };

// frozen reference state of an orthogonality slot (gpe_bind_orth_state): a parameter set of the engine's own network, in the engine's
// (padded) layout, with its packed copies, and psi_k on the collocation set bound now -- orth_host[k] points at psi
struct OrthState {
    bool on = false;
    float *theta = nullptr, *Wpk = nullptr, *WpkT = nullptr;
    float* psi = nullptr;          // [n]
    int64_t n = 0;
    int base_mode = -1;
    float perturb_scale = 1.f, amplitude = 1.f, base_norm = 1.f;
};

// what the caller of a step's phases promises about how it enqueues them
struct StepOpts {
    bool head_may_fuse = false;    // nobody reads the step sums between the passes: the head may ride in the forward kernel
    bool update_may_fuse = false;  // reduction and update are enqueued back to back: the update may ride in the slab reduction
    bool capturing = false;        // graph_build is recording: neither count the step nor redraw
};
// what the phases of one step hand to the next; e->st = StepState{} is the only reset
struct StepState {
    int phase = 0;                 // 0 idle, 1 after begin, 2 after backward, 3 after mse begin
    bool bc_inflight = false;      // the boundary batch was forked: its gradient (grad_bc) waits for the reverse pass that closes the step
    int head_slots = 0;            // the forward pass left this many per-workgroup head triples in head_slots (= its workgroups); 0: k_head_pde ran
    bool update_done = false;      // the update already ran inside the slab reduction
    bool update_parts = false;     // the slab reduction left partial norms + snapshot for the multi-workgroup update
};
// one reverse pass (mlp_backward)
struct BwdOpts {
    bool close = false;            // the last reverse pass of the step: join the boundary batch, add its gradient, write the exchange tail
    bool assign = true;            // the first one: the gradient is assigned, not accumulated
    bool seeds_in_kernel = false;  // small batch: the pipelined kernel forms the seeds itself (k_seed_pde was not launched)
    bool update_may_fuse = false;  // StepOpts::update_may_fuse
    bool bucketed = false;         // data-parallel step, generic set: finished layers go to the exchange stream
};

// What the records of an engine look like -- struct gpe_observables or struct gpe_mixture_observables: an engine is scalar or mixture
// for life (gpe_observe.h, gpe_observe_mix.h)
struct ObsKind {
    int rec_doubles, row;          // doubles per record / per slab row of its reduction chain
    int f_energy, f_res;           // index of the double a keeper judges by GPE_KEEP_ENERGY / GPE_KEEP_RES_RMS
};
#define OBS_FIELD(R, f) (int)(offsetof(struct R, f) / sizeof(double))
static const ObsKind OBS_SCALAR = {(int)(sizeof(struct gpe_observables) / sizeof(double)), OB_ROW, OBS_FIELD(gpe_observables, energy),
                                   OBS_FIELD(gpe_observables, res_rms)};
static const ObsKind OBS_MIXTURE = {(int)(sizeof(struct gpe_mixture_observables) / sizeof(double)), MO_ROW, OBS_FIELD(gpe_mixture_observables, energy),
                                    OBS_FIELD(gpe_mixture_observables, res_rms_total)};
#undef OBS_FIELD

struct gpe_engine {
    gpe_config cfg;
    NetDesc nd;
    Phys ph;
    OptCfg oc;
    int device = 0;
    hipStream_t stream = nullptr;
    int path = GPE_PATH_GENERIC;
    int H = 0;                     // uniform hidden width (fused)
    bool wide = false;             // fused path: reverse pass by the wide kernel set (gpe_wide.h): H = 256 or 128
    bool wide_fwd = false;         // ... and the forward pass too (H = 256, H = 128 in 3D; H = 128 in 1D/2D keeps f_forward_coop: measured)
    int64_t gen_min_chunk = 32;    // generic set, split-K weight gradient on the matrix cores: fewest points per wave (GPE_GEN_MIN_CHUNK; 256 before round 4)
    int64_t wide_min_tiles = 2048; // H = 128 in 1D/2D: batches below this many 16-point tiles take the single-launch cooperative reverse kernel
    int P = 0, Ppad = 0;
    // width padding: hidden widths without an MFMA kernel instance run zero-padded to the next width that has one.  P counts the
    // padded network (what the kernels, the optimiser and the gradient exchange see); the caller's flat vector has P_user entries
    // and umap[i] is the padded index of its i-th entry.  Empty map: no padding, P_user == P.
    int P_user = 0;
    std::vector<int> umap;
    std::vector<int> pad_bias;     // ShiftedTanh: biases of the padded units (held at -40: tanh = -1 exactly, so the unit outputs 0 with zero slope)
    int user_layers[GPE_MAX_LAYERS] = {0};
    float base_norm = 1.f;
    float *theta = nullptr, *am = nullptr, *av = nullptr, *grad = nullptr;   // grad: P + GT_COUNT
    double* dbl = nullptr;         // [S_COUNT sums | LS_COUNT local | 4 misc]
    OptDev* od = nullptr;
    bool update_cache = true;      // single-workgroup update: register-cached elements + scatter packing (GPE_UPDATE_CACHE=0: the two-pass form)
    bool fuse_seed = true;         // small batches: the pipelined reverse kernel forms the seeds itself (GPE_FUSE_SEED=0: k_seed_pde)
    int64_t fuse_seed_max = 65536; // ... up to this many points (beyond, the redundant seed arithmetic of the four waves costs more than the launch)
    int share_min_tiles = 16;      // ... for batches of at least this many tiles per workgroup (per wave in the forward kernel)
    int fwd_share = 640;           // f_forward: the same for its waves (GPE_FWD_SHARE; measured flat between 608 and 672: NS step 2.703 -> 2.688 ms)
    int pipe_share = 576;          // f_backward_pipe: share (/1024) of a CU's tiles for its first-dispatched workgroup; 0 = even (GPE_PIPE_SHARE;
                                   // NS reverse kernel 1.741 ms even, 1.727 / 1.719 / 1.715 / 1.730 / 1.741 ms at 544 / 576 / 592 / 608 / 640)
    bool fuse_head = true;         // ... and the cooperative forward kernel runs the head (GPE_FUSE_HEAD=0: k_head_pde): whole steps only,
    int64_t fuse_head_max = 6144;  // up to this many points (measured: 43.2 vs 46.5 us at 4 000, equal at 6 000, 64.3 vs 62.9 us at 8 192)
    int64_t fuse_head_tile_min = 32769;   // f_forward (per-wave tiles) runs the head from this many points on (GPE_FUSE_HEAD_TILE_MIN)
    double* head_slots = nullptr;  // [HEAD_SLOTS][4]
    bool fuse_update = false;      // small P, whole steps: the last-arriving workgroup of the slab reduction runs the update (k_reduce_update; opt-in GPE_FUSE_UPDATE=1)
    unsigned* upd_ticket = nullptr;
    bool split_update = false;     // small P, whole steps: slab reduction in the update's partition + k_update<true> on UPD_G workgroups (opt-in GPE_SPLIT_UPDATE=1)
    UpdSnap* upd_snap_small = nullptr;
    UpdSnap* upd_snap = nullptr;   // multi-workgroup update (P >= UPD_MULTI_MIN): partial norms + snapshot of sums / optimiser state
    gpe_scalars *hist = nullptr, *last = nullptr;
    int cap = 65536;
    float *Wpk = nullptr, *WpkT = nullptr, *gslab = nullptr;
    int nslab = 0;
    bool packed_dirty = true;
    bool acc_clean = false;                       // step sums are zero (left so by k_update): the next step needs no k_begin
    bool ext_exchange = false;
    bool fwd_wlds = false;                        // forward kernel stages the hidden-hidden weights in LDS
    bool fwd_b6 = false;                          // f_forward_b6: H x H maps as six bf16 MFMA products per fp32 product (H <= 64; GPE_FWD_B6)
    bool bwd_b6 = false;                          // f_backward_coop<..., B6>: the adjoint products the same way (H <= 64; GPE_BWD_B6)
    int coop_wg_per_cu = 2;                       // cooperative reverse kernels at H <= 64: persistent workgroups per CU (tuning: GPE_COOP_WG_PER_CU)
    int fwd_wg_per_cu = 2;                        // per-wave-tile forward kernel: persistent workgroups per CU (tuning: GPE_FWD_WG_PER_CU; 3 needs a -DGPE_FWD_WAVES=3 build)
    bool bwd_pipe = true;                         // cooperative reverse kernel in its one-barrier-per-map form (f_backward_pipe; H <= 64; GPE_PIPE)
    bool bwd_racc = false;                        // reverse kernel keeps the H x H weight gradients in registers (1 wave/SIMD)
    int nslab_g = 16;                             // H = 128: number of global-atomic gradient slabs
    int coop = 1;                                 // cooperative reverse kernel: 0 never, 1 whenever compiled for the shape, -1 by batch size
    int64_t coop_max_tiles = 0;
    bool coop_fwd128 = true;
    bool gen_mfma2 = true;                        // ... with 128 x 128 block tiles and LDS-shared operand panels
    bool gen_mfma = true;                         // generic path: MFMA split-K weight gradient for wide layers
    bool coop128 = true;                          // H = 128: use the cooperative reverse kernel (else global-atomic slabs)
    int64_t coop_fwd_max_tiles = 0;               // forward: cooperative kernel for batches up to this many tiles
    int64_t stage_min_tiles = 0;                  // batches with fewer 16-point tiles use the unstaged kernels (latency-bound regime)
    hipStream_t side = nullptr;                   // boundary batch runs here, concurrently with the collocation batch
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    float *gslab_bc = nullptr, *grad_bc = nullptr;
    // gpe_run replays one captured step (hipGraph) while every by-value launch argument is unchanged
    bool use_graph = false;
    int graph_steps = 8;           // steps captured per graph (GPE_GRAPH_STEPS)
    bool graph_forced = false;     // GPE_GRAPH set: at every batch size; otherwise only up to graph_max_points
    int64_t graph_max_points = 16384;
    hipStream_t cap_stream = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    std::vector<char> graph_key;
    bool prof = false;
    std::vector<hipEvent_t> ev_pool;      // pairs: [2i] start, [2i+1] stop
    std::vector<int> ev_kind;             // 0 forward, 1 reverse
    size_t ev_used = 0;
    const float** orth_dev = nullptr;
    const float* orth_host[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [4..6]: precomputed base
    Batch main, bc, sym, aux, mse;
    OrthState ost[GPE_MAX_ORTH];   // frozen states: evaluated by the engine on every set it holds (orth_refill)
    Batch orb;                     // ... through this value-only forward batch on the collocation points, sized at the binds
    const float* bc_target = nullptr;
    // what the caller bound: collocation points / potential, boundary points.  When the boundary batch is small it is MERGED:
    // appended to the collocation batch (main.pts.b) and handled by the same launches; e->bc stays empty then.
    const float* ux = nullptr; const float* uV = nullptr; const float* uxb = nullptr;
    int64_t n_pde = 0, nb_user = 0, nb_merged = 0;
    bool merge_bc = true;
    const float* mse_target = nullptr;
    int num_cu = 256;
    int head_wg_per_cu = 1;        // head / seed kernels: workgroups per CU (each ends in one double atomic per global sum: ~22 ns apiece at one address)
    int head_threads = 1024;       // ... and threads per workgroup (GPE_HEAD_THREADS; 256 x 2 per CU until round 3: half the loads in flight, twice the atomics)
    // ---- data-parallel exchange inside the engine: RCCL on a dedicated stream (gpe_comm_init); gpe_comm_destroy resets all of it ----
    struct Dp {
        struct Rccl {
            void* dl = nullptr;
            ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
            ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
            ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
            ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
            const char* (*GetErrorString)(ncclResult_t) = nullptr;
        } rccl;
        ncclComm_t comm = nullptr;
        int rank = 0, world = 1;
        hipStream_t stream = nullptr;                     // the exchange stream
        hipEvent_t ev_x0 = nullptr, ev_x1 = nullptr;      // compute -> exchange, exchange -> compute
        std::vector<hipEvent_t> ev_bucket;                // one per linear map: its gradient slice is final
        // opt-in one-step-stale gradient (gpe_comm_set_async): the all-reduce of g_t runs on the exchange stream behind the forward of
        // step t+1, whose update applies g_t; changes the trajectory -- never on by default
        bool async_grad = false;
        float* grad_alt = nullptr;                        // second gradient buffer (P + GT_COUNT)
        double* dbl_prev = nullptr;                       // sums of the step whose gradient is in flight
        hipEvent_t ev_g[2] = {nullptr, nullptr};
        int64_t async_t = 0;
        int64_t collectives = 0;                          // all-reduces issued since gpe_comm_init (bench / tests)
        bool inline_sync = true;                          // synchronous step on the fused / wide sets: collectives on the compute stream (GPE_DP_INLINE=0: exchange stream)
        bool on() const { return comm != nullptr; }
        bool async() const { return async_grad; }
    } dp;
    // ---- observables (gpe_observe.h) ----
    const ObsKind* obs_kind = nullptr;                // the engine's kind of record, chosen at the create for life
    double* obs_buf = nullptr;                        // [pass-1 slab | pass-2 slab | raw totals], allocated on first use
    double* obs_out = nullptr;                        // staging slot of gpe_observables / gpe_mixture_observables: one record of the engine's kind
    // held-out monitor (gpe_bind_monitor): its own forward batch, sized at the bind -- gpe_run must neither allocate nor synchronise
    struct Monitor {
        Batch b;
        const float* x = nullptr; const float* V = nullptr;
        float* Vown = nullptr;                        // [n]: V of the monitor's set as the bound potential terms give it (V points here), else NULL
        float dv = 0.f;
        int64_t n = 0, every = 0;                     // every == 0: no monitor
        int64_t steps = 0, records = 0;               // steps enqueued / records appended since the bind
        int cap = 0;
        double* ring = nullptr;                       // [cap] records of the engine's kind
        bool bound() const { return every > 0; }
        int64_t room() const { return every - steps % every; }      // steps up to and including the next record's (bound() only)
    } mon;
    // keeper (gpe_bind_keeper): the best parameters by one field of the monitor's records; both buffers allocated at the bind
    struct Keeper {
        int metric = GPE_KEEP_NONE;                   // GPE_KEEP_NONE: no keeper
        double min_delta = 0.0;
        int64_t patience = 0;
        float* theta_best = nullptr;                  // [P], the engine's own padded layout
        KeepDev* dev = nullptr;
        bool armed() const { return metric != GPE_KEEP_NONE; }
    } keep;
    // device-side stratified sampler (gpe_bind_sampler and its kin): the engine owns the collocation points and redraws them in place.
    // One record for the four kinds; what is allocated says which one is bound (the predicates), and sampler_free resets all of it.
    struct Sampler {
        float* x = nullptr;                               // [n][dim]; ux points here while a sampler is bound
        SamplerGrid grid = {};
        int64_t n = 0, first = 0, every = 0;              // rows, first cell (or first row of the list); every == 0: no sampler
        int64_t draw0 = 0, held = 0;                      // draw at the bind / draw the buffer holds (as enqueued)
        int64_t steps = 0;                                // steps enqueued since the bind
        // graded (gpe_bind_sampler_graded; the adaptive sampler, and the cell-subset sampler given edges, are graded too): the cell edges
        // of every axis, one after the other, and the engine-owned weights
        float* edges = nullptr;                           // [sum_k shape[k] + 1]; axis k starts at edge_off[k]
        int64_t edge_off[3] = {0, 0, 0};
        float* q = nullptr;                               // [n] cell volumes; wq points here while a graded sampler is bound
        // residual-adaptive (gpe_sampler_adaptive): the cells are blocks of varying row counts; every buffer is allocated at the bind
        struct Adaptive {
            AdaptiveDev dev = {};                         // mass [B + 1], count [B], off [B + 1], vol [B], share [B] and the allocation's constants
            float* vol = nullptr;                         // (dev.vol, writable)
            float* resid = nullptr;                       // [n][n_out]: the residual of the set held, written by the detour before a redraw
        } ad;
        // cell subset (gpe_sampler_cells): the rows are [first, first + n) of a list of cells, uniform or graded
        struct Cells {
            int64_t* list = nullptr;                      // [n] strictly ascending row-major cell indices
            int64_t n = 0;
        } cl;
        double* wq_red = nullptr;                         // [2] output of k_weight_total: scratch of every weight bind, allocated at the first, kept until the engine goes
        bool bound() const { return every > 0; }
        bool graded() const { return edges != nullptr; }
        bool adaptive() const { return ad.dev.mass != nullptr; }      // (implies graded)
        bool cells() const { return cl.list != nullptr; }             // (excludes adaptive)
    } smp;
    // per-point quadrature weights (gpe_bind_weights): every collocation sum takes q_i, every N of a mean becomes W (Phys::n_global)
    const float* wq = nullptr;                        // [n_pde]: the caller's array, or smp.q; NULL: unweighted
    double wq_local = 0.0, wq_total = 0.0;            // sum of this rank's weights / W over all ranks
    // analytic potential terms (gpe_potential_terms, gpe_potential.h): the engine owns V of the sets it holds and fills it from the table
    struct PotTerms {
        PotTable tab = {};                            // the table, by value into k_potential_terms
        int n = 0;                                    // terms bound; 0: none
        float* V = nullptr; int64_t nV = 0;           // V of the bound collocation set; uV points here while that set runs on the engine's V
        float* Vtmp = nullptr; int64_t nVtmp = 0;     // scratch of one-off observables on other points, grown on demand
        bool on() const { return n > 0; }
    } pot;
    bool pot_bound() const { return pot.V && uV == pot.V && ux; }      // the bound set runs on the engine's V
    float mix_wE = 0.f;                               // mixture energy term (gpe_mixture_energy_weight): its weight, 0 = the plain mixture step
    // device-resident L-BFGS (gpe_lbfgs.h): every buffer allocated by gpe_lbfgs_config, freed with the engine
    struct Lbfgs {
        bool on = false;
        LbfgsCfg cfg = {};
        int ld = 0, n_part = 0;
        struct Hist {                                                             // a new `history` (cfg.m) reallocates this alone, cleared
            float *S = nullptr, *Y = nullptr, *g_prev = nullptr, *d = nullptr;    // rings [m][ld]; [ld] each
            double *part = nullptr, *SY = nullptr, *YY = nullptr, *ro = nullptr, *coef = nullptr;
        } h;
        LbfgsDev* st = nullptr;
        LsCfg ls = {};                                                            // strong-Wolfe line search (gpe_lbfgs_line_search); kind 0: none
        float* ls_buf = nullptr;                                                  // [4][ld]: three trial-gradient slots, theta0
        double* ls_part = nullptr;                                                // [n_part][LSD_COUNT]
        bool mon = false;                                                         // gpe_lbfgs_monitor: gpe_lbfgs_run serves the monitor
        float* view_buf = nullptr;                                                // [ld]: theta, set aside during a monitor tick
    } lb;
    StepState st;
    std::string err;
    double* sums() { return dbl; }
    double* lsums() { return dbl + S_COUNT; }
    double* dsc() { return dbl + DBL_COUNT - 4; }
};

// Every launcher enqueues on e->stream and writes the gradient through e->grad / e->gslab.  The boundary batch (side stream, grad_bc),
// the stale-gradient step (alternating buffer) and the graph capture (capture stream) send them elsewhere for a while: only through
// this guard, which puts the engine's own back on every way out.
struct Redirect {
    gpe_engine* e; hipStream_t stream; float *grad, *gslab;
    Redirect(gpe_engine* e_, hipStream_t s, float* g, float* sl) : e(e_), stream(e->stream), grad(e->grad), gslab(e->gslab) { e->stream = s; e->grad = g; e->gslab = sl; }
    ~Redirect() { e->stream = stream; e->grad = grad; e->gslab = gslab; }
    Redirect(const Redirect&) = delete;
};
// The per-step record lives from one phase to the next only: a sequence clears it on every way out -- a step that failed half-way
// must not leave anything behind -- except where it hands the record on to the next phase (keep).
struct StepScope {
    gpe_engine* e; bool kept = false;
    ~StepScope() { if (!kept) e->st = StepState{}; }
    int keep() { kept = true; return GPE_OK; }
};

static void free_batch(Batch& b) {
    for (void* p : b.allocs) (void)hipFree(p);
    b = Batch();
}

template <typename T>
static int dev_alloc(gpe_engine* e, Batch* b, T** out, size_t count) {
    void* p = nullptr;
    HIPCHK(e, hipMalloc(&p, count * sizeof(T) + 256));
    HIPCHK(e, hipMemsetAsync(p, 0, count * sizeof(T) + 256, e->stream));
    if (b) b->allocs.push_back(p);
    *out = (T*)p;
    return GPE_OK;
}

// one device record as the work enqueued so far leaves it, to the host -- or replaced from the host; every reader and writer synchronises here
template <typename T>
static int record_copy(gpe_engine* e, T* dst, const T* src, hipMemcpyKind kind) {
    HIPCHK(e, hipMemcpyAsync(dst, src, sizeof(T), kind, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

static int setup_batch(gpe_engine* e, Batch& b, const float* x, int64_t n, int C, int E, bool with_head, const float* V,
                       bool with_store = true) {
    if (b.n == n && b.C == C && b.E == E && b.O) { b.pts = Pts{x, nullptr, n}; b.V = V; return GPE_OK; }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    free_batch(b);
    b.pts = Pts{x, nullptr, n}; b.V = V; b.n = n; b.C = C; b.E = E;
    b.ld = round_up(n, 64);
    const int no = e->nd.n_out;
    int rc;
    if ((rc = dev_alloc(e, &b, &b.O, (size_t)C * no * b.ld))) return rc;
    if ((rc = dev_alloc(e, &b, &b.Ob, (size_t)C * no * b.ld))) return rc;
    if (with_head) {
        if ((rc = dev_alloc(e, &b, &b.u, (size_t)no * b.ld))) return rc;
        if ((rc = dev_alloc(e, &b, &b.Hu, (size_t)no * b.ld))) return rc;
        if ((rc = dev_alloc(e, &b, &b.ux, (size_t)no * e->nd.dim * b.ld))) return rc;      // [n_out][dim][ld]
    }
    const int L = e->nd.n_lin - 1;
    if (e->path == GPE_PATH_FUSED) {
        int64_t ntiles = (n + 15) / 16;
        size_t cnt = with_store ? (size_t)ntiles * (L - 1) * C * e->H * 16 : 0;     // forward-only batches keep nothing
        if ((rc = dev_alloc(e, &b, &b.stored, cnt ? cnt : 4))) return rc;
        if (e->wide && with_store) {
            const size_t zc = (size_t)ntiles * C * e->H * 16;
            if ((rc = dev_alloc(e, &b, &b.Z0, zc))) return rc;
            if ((rc = dev_alloc(e, &b, &b.Z1, zc))) return rc;
        }
    } else {
        int maxW = 1;
        for (int h = 0; h < L; ++h) {
            float* s;
            if ((rc = dev_alloc(e, &b, &s, (size_t)C * e->nd.width[h + 1] * b.ld))) return rc;
            b.S.push_back(s);
            if (e->nd.width[h + 1] > maxW) maxW = e->nd.width[h + 1];
        }
        if ((rc = dev_alloc(e, &b, &b.A0, (size_t)C * maxW * b.ld))) return rc;
        if ((rc = dev_alloc(e, &b, &b.A1, (size_t)C * maxW * b.ld))) return rc;
        if (e->cfg.net_kind == GPE_NET_RESIDUAL && (rc = dev_alloc(e, &b, &b.A2, (size_t)C * maxW * b.ld))) return rc;
    }
    return GPE_OK;
}

// ---- MLP forward / backward dispatch ---------------------------------------------------------------
// gpe_dispatch.h holds the table: the (C, E) pairs that exist, the n_out values, and each fused kernel form with its template ranges.
// Every launcher below picks its template arguments through it, one statement per kernel form; raise_lds_limits walks the same ranges.
#ifdef GPE_FAST_BUILD    // kernel-tuning builds (tools/build_variant.sh): only what the 2D / 3D n_out = 1, H = 64 workloads launch
#define BAD_CE "fast build: channels (%d,%d) not compiled"
#else
#define BAD_CE "bad channel pair (%d,%d)"
#endif
// f(CC, EE) for the batch's channel pair out of `list`, or the error
template <class L, class F>
static int launch_ce(gpe_engine* e, const Batch& b, L list, F&& f) {
    if (!pick_ce(list, b.C, b.E, f)) FAIL(e, GPE_ERR_INVALID, BAD_CE, b.C, b.E);
    return GPE_OK;
}
// f(HH, CC, EE) for the fused kernels: H = 32 / 64 with the pairs of L, H = 128 with those of L128
template <class L, class L128, class F>
static int launch_hce(gpe_engine* e, const Batch& b, F&& f) {
#ifdef GPE_FAST_BUILD
    if (e->H != 64 || e->nd.n_out != 1) FAIL(e, GPE_ERR_INVALID, "fast build: only H = 64, n_out = 1 compiled");
#else
    if (e->H == 128) {
        if (!pick_ce(L128{}, b.C, b.E, [&](auto CC, auto EE) { f(int_c<128>{}, CC, EE); })) FAIL(e, GPE_ERR_INVALID, BAD_CE " for H = 128", b.C, b.E);
        return GPE_OK;
    }
    if (e->H == 32) return launch_ce(e, b, L{}, [&](auto CC, auto EE) { f(int_c<32>{}, CC, EE); });
#endif
    return launch_ce(e, b, L{}, [&](auto CC, auto EE) { f(int_c<64>{}, CC, EE); });
}

static size_t fused_w_bytes(gpe_engine* e) { return (size_t)(e->nd.n_lin - 2) * e->H * e->H * sizeof(float); }
static size_t fused_small_bytes(gpe_engine* e) {       // = small_count() of gpe_fused.h, rounded up to 16 bytes (NOT read_switches' smallb, on purpose)
    size_t n = (size_t)(4 + (e->nd.n_lin - 2) + e->nd.n_out) * e->H + 4;
    return ((n + 3) & ~(size_t)3) * sizeof(float);
}
static bool staged_batch(gpe_engine* e, const Batch& b) { return (b.n + 15) / 16 >= e->stage_min_tiles; }
static size_t fused_fwd_lds(gpe_engine* e, bool staged) { return fused_small_bytes(e) + (e->fwd_wlds && staged ? fused_w_bytes(e) : 0); }

static bool coop_shape(gpe_engine* e);
static unsigned fused_grid(gpe_engine* e, int64_t n, int waves_per_block, int blocks_per_cu);
// residual blocks on the fused path: only the cooperative kernels (<..., RES>) implement the skip connection -- they run whatever
// GPE_COOP says (the per-wave-tile kernels would evaluate a plain MLP)
static bool coop_only(gpe_engine* e) { return coop_shape(e) && e->H <= 64 && e->cfg.net_kind == GPE_NET_RESIDUAL; }
static bool fwd_coop(gpe_engine* e, const Batch& b) {
    if (coop_only(e)) return true;
    if (!coop_shape(e) || e->coop == 0) return false;
    if (e->H == 128) return e->coop_fwd128 && b.C <= 4;      // wide layers: the cooperative forward wins at every size (measured); gpe_forward_jets' (5,2) has no instance
    if (e->nd.n_lin - 2 > 3) return true;             // four / five maps at H <= 64: the cooperative kernels take them whenever allowed
    return (b.n + 15) / 16 <= e->coop_fwd_max_tiles;
}
// workgroups of the forward launch of batch b: cooperative (a workgroup per tile, two per CU) or per wave tile (four tiles per workgroup);
// H = 128 runs one workgroup per CU either way.  The head leaves one triple per workgroup of this launch (step_begin).
static unsigned fwd_grid(gpe_engine* e, const Batch& b, bool coop) {
    return fused_grid(e, b.n, coop ? 1 : 4, e->H == 128 ? 1 : (coop ? 2 : e->fwd_wg_per_cu));
}
// large batches on two workgroups per CU: uneven split of each CU's tiles between its two workgroups, / 1024 (0: even).  Forward
// (GPE_FWD_SHARE; per wave, hence the 4) and pipelined reverse (GPE_PIPE_SHARE); gpe_active_kernels reports what these return.
static int fwd_tile_share(gpe_engine* e, const Batch& b, unsigned grid) {
    return (e->fwd_share > 0 && grid == (unsigned)(2 * e->num_cu) && (b.n + 15) / 16 >= 4 * e->share_min_tiles * (int64_t)grid) ? e->fwd_share : 0;
}
static int pipe_tile_share(gpe_engine* e, const Batch& b, unsigned grid) {
    return (e->pipe_share > 0 && grid == (unsigned)(2 * e->num_cu) && (b.n + 15) / 16 >= e->share_min_tiles * (int64_t)grid) ? e->pipe_share : 0;
}
#define HEAD_SLOTS 512
static bool seed_in_reverse(gpe_engine* e);
// no Riesz term, Rayleigh-quotient eigenvalue, no regularisers: the loss the fused head / seed code paths implement
static bool plain_terms(const gpe_engine* e) {
    return e->cfg.w_riesz == 0.f && e->cfg.lambda_kind == GPE_LAMBDA_RAYLEIGH && e->cfg.w_reg_f == 0.f && e->cfg.w_reg_lam == 0.f;
}
// problem class whose head the forward kernels can run (head_point_real): real psi, no orthogonality / Riesz / symmetry terms, no
// quadrature weights
static bool head_class(gpe_engine* e) {
    return e->fuse_head && !e->wq && e->head_slots && e->path == GPE_PATH_FUSED && !e->wide && e->H <= 64 && e->nd.n_out == 1 && !e->cfg.complex_psi &&
           e->ph.n_orth == 0 && plain_terms(e) && e->cfg.w_sym == 0.f && e->main.C >= 3 && e->main.n > 0;
}
// ... by the cooperative forward kernel (small batches; the reverse kernel forms the seeds and adds the triples)
static bool head_fusable_coop(gpe_engine* e) {
    // (four / five maps and residual blocks have no seed-forming reverse kernel: k_seed_pde adds their triples, as it does for large batches)
    const bool deep = e->nd.n_lin - 2 > 3 || e->cfg.net_kind == GPE_NET_RESIDUAL;
    return head_class(e) && e->main.n <= e->fuse_head_max && fwd_coop(e, e->main) && (seed_in_reverse(e) || deep) && fused_grid(e, e->main.n, 1, 2) <= HEAD_SLOTS;
}
// ... by the per-wave-tile forward kernel (large batches; k_seed_pde, or the seed-forming reverse kernel, adds the triples)
static bool head_fusable_tile(gpe_engine* e) {
    return head_class(e) && !fwd_coop(e, e->main) && !e->fwd_b6 && e->main.n >= e->fuse_head_tile_min && fused_grid(e, e->main.n, 4, e->fwd_wg_per_cu) <= HEAD_SLOTS;
}
static bool head_fusable(gpe_engine* e) { return head_fusable_coop(e) || head_fusable_tile(e); }
// head: the kernel runs the head too and leaves one triple per workgroup in head_slots (the step's forward pass of the main batch only)
static HeadArgs head_args(gpe_engine* e, const Batch& b) {
    return HeadArgs{e->ph, e->base_norm, b.V, (const float* const*)e->orth_dev, e->bc_target, b.u, b.Hu, b.Ob, e->n_pde, b.ld, e->head_slots};
}
template <int HH, int CC, int EE>
static void launch_f_forward_coop(gpe_engine* e, Batch& b, int store, const FwdWeights& W, bool head) {
    constexpr int NT = HH / 16;
    const int maps = e->nd.n_lin - 2;
    pick_n_out(e->nd.n_out, [&](auto no) {
        constexpr int NO = decltype(no)::value;
        const bool hd = head && head_form(HH, CC, NO), res = e->cfg.net_kind == GPE_NET_RESIDUAL && HH <= 64 && NO == 1;
        const HeadArgs ha = hd ? head_args(e, b) : HeadArgs{};
        const size_t lds = fused_small_bytes(e) + ((size_t)2 * CC * NT * 256 + (size_t)NT * e->nd.n_out * CC * 16 + (hd ? CC * 16 : 0)) * sizeof(float);
        // one or two residual blocks (checked at gpe_create) are two or four maps
        pick_int<1, 5>(res ? (maps == 2 ? 2 : 4) : maps, [&](auto nh) { pick_int<0, 1>(hd, [&](auto h) { pick_int<0, 1>(res, [&](auto r) {
            constexpr int NH = decltype(nh)::value;
            constexpr bool HEAD = decltype(h)::value, RES = decltype(r)::value;
            if constexpr (coop_form(HH, NO, NH, RES) && (!HEAD || head_form(HH, CC, NO)))
                hipLaunchKernelGGL((f_forward_coop<HH, CC, EE, NO, NH, HEAD, RES>), dim3(fwd_grid(e, b, true)), dim3(HH * 4), lds, e->stream,
                                   e->nd, W.theta, W.Wpk, b.pts, b.stored, b.O, b.n, b.ld, store, ha);
        }); }); });
    });
}
template <int HH, int CC, int EE>
static void launch_f_forward(gpe_engine* e, Batch& b, int store, const FwdWeights& W, bool head) {
    if constexpr (HH <= 64 || CC <= 4) if (fwd_coop(e, b)) return launch_f_forward_coop<HH, CC, EE>(e, b, store, W, head);
    const unsigned grid = fwd_grid(e, b, false);
    const bool staged = HH <= 64 && staged_batch(e, b);
    pick_n_out(e->nd.n_out, [&](auto no) {
        constexpr int NO = decltype(no)::value;
        if (staged && e->fwd_b6) {
            // weights (three bf16 pieces, 6 bytes each) in LDS when two workgroups per CU still fit
            const size_t w6 = (size_t)(e->nd.n_lin - 2) * HH * HH * 6;
            pick_int<0, 1>(2 * (fused_small_bytes(e) + w6) <= (size_t)160 * 1024, [&](auto w) {
                constexpr bool WL = decltype(w)::value;
                if constexpr (HH <= 64)
                    hipLaunchKernelGGL((f_forward_b6<HH, CC, EE, NO, WL>), dim3(grid), dim3(256), fused_small_bytes(e) + (WL ? w6 : 0), e->stream,
                                       e->nd, W.theta, W.WpkT, b.pts, b.stored, b.O, b.n, b.ld, store);
            });
            return;
        }
        const bool hd = head && head_form(HH, CC, NO);       // whole step, large batch: the head rides in this kernel
        const HeadArgs ha = hd ? head_args(e, b) : HeadArgs{};
        pick_int<0, 1>(staged && e->fwd_wlds, [&](auto w) { pick_int<0, 1>(hd, [&](auto h) {
            constexpr bool WL = decltype(w)::value, HEAD = decltype(h)::value;
            if constexpr (!HEAD || head_form(HH, CC, NO))      // (WL is compiled at H = 128 too, and never picked there: staged)
                hipLaunchKernelGGL((f_forward<HH, CC, EE, NO, WL, HEAD>), dim3(grid), dim3(256), fused_fwd_lds(e, WL), e->stream,
                                   e->nd, W.theta, W.Wpk, b.pts, b.stored, b.O, b.n, b.ld, store, fwd_tile_share(e, b, grid), ha);
        }); });
    });
}
// reverse-kernel variant for one batch: 3 = cooperative (a workgroup per tile, a wave per 16-feature slice),
// 2 = weight gradients in registers (1 wave/SIMD),
// 0 = plain (LDS-atomic gradients, weights from L2; also the fastest when every wave sees only a tile or two)
static bool coop_shape(gpe_engine* e) {
    if (e->path != GPE_PATH_FUSED) return false;
    const int maps = e->nd.n_lin - 2;                 // hidden -> hidden maps
    // H <= 64: one to three maps on the pipelined / cooperative kernels; round 4: FOUR and FIVE maps (real psi) on the cooperative ones too -- the
    // per-wave-tile kernels cannot hold a fourth map's weight gradient in registers, nor its weights in 64 KB of LDS, and ran such networks 2.4-3x
    // slower per FLOP (profiles/r04/deep_h64_networks.txt)
    if (e->H <= 64) return maps >= 1 && maps <= (e->nd.n_out == 1 ? 5 : 3);
    return e->H == 128 && maps >= 1 && maps <= 5 && e->nd.dim <= 2 && e->coop128;    // 8 waves per workgroup, weights streamed from L2
}
static int bwd_kind(gpe_engine* e, const Batch& b);
static bool use_pipe(gpe_engine* e, int C);
// small batches of the common problem class (real psi, no orthogonality / Riesz / symmetry terms) on the pipelined reverse kernel:
// the kernel forms the seeds itself and k_seed_pde is not launched (bound quadrature weights keep k_seed_pde: the fused seeds have none)
static bool seed_in_reverse(gpe_engine* e) {
    return e->fuse_seed && !e->wq && e->path == GPE_PATH_FUSED && !e->wide && e->nd.n_out == 1 && !e->cfg.complex_psi && e->ph.n_orth == 0 &&
           plain_terms(e) && e->cfg.w_sym == 0.f && e->main.C >= 3 && e->main.n > 0 && e->n_pde <= e->fuse_seed_max &&
           use_pipe(e, e->main.C) && bwd_kind(e, e->main) == 3;
}
// H = 128 in 1D / 2D has two reverse passes behind the cooperative forward kernel (same stored-activation format): one launch per map
// (w_bwd_map: no spills, -3.6 % at 4 096 tiles) and the single cooperative launch (f_backward_coop<128>: fewer launches, -10 % at 256
// tiles, -4 % at 1 024; profiles/r04/wide_small_batch_ab.txt).  The per-map form from wide_min_tiles tiles on (GPE_WIDE_MIN_TILES).
static bool wide_reverse(gpe_engine* e, const Batch& b);
static int bwd_kind(gpe_engine* e, const Batch& b) {
    if (coop_only(e)) return 3;
    if (coop_shape(e) && e->coop != 0 && (e->coop == 1 || (b.n + 15) / 16 <= e->coop_max_tiles || (e->H <= 64 && e->nd.n_lin - 2 > 3))) return 3;
    if (e->H > 64 || !staged_batch(e, b)) return 0;
    return e->bwd_racc ? 2 : 0;
}
static bool wide_reverse(gpe_engine* e, const Batch& b) {
    if (!e->wide) return false;
    if (e->wide_fwd || e->H != 128 || e->nd.dim > 2) return true;              // H = 256, 3D: the wide set is the only one
    return (b.n + 15) / 16 >= e->wide_min_tiles || bwd_kind(e, b) != 3;
}
// f_backward_pipe: two z and two X^T exchange buffers; taken when two workgroups per CU still fit
static size_t pipe_lds(gpe_engine* e, int C) {
    const int H = e->H, NT = H / 16, L = e->nd.n_lin - 1;
    const size_t n_gsm = ((size_t)(L - 1 + e->nd.n_out) * H + 4 + 3) & ~(size_t)3;
    return (n_gsm + 4 * (size_t)H) * sizeof(float) + fused_small_bytes(e) + (size_t)4 * C * NT * 256 * sizeof(float);
}
static bool use_pipe(gpe_engine* e, int C) {
    return e->bwd_pipe && !e->bwd_b6 && e->H <= 64 && e->cfg.net_kind == GPE_NET_MLP && e->nd.n_lin - 2 >= 1 && e->nd.n_lin - 2 <= 3 && 2 * (pipe_lds(e, C) + 1024) <= (size_t)160 * 1024;
}
static size_t coop_lds(gpe_engine* e, int C) {
    if (use_pipe(e, C)) return pipe_lds(e, C);
    const int H = e->H, NT = H / 16, L = e->nd.n_lin - 1;
    const size_t n_gsm = ((size_t)(L - 1 + e->nd.n_out) * H + 4 + 3) & ~(size_t)3;
    const size_t zb = e->bwd_b6 && H <= 64 ? (size_t)3 * C * (NT / 2) * 256 : (size_t)C * NT * 256;     // B6: three bf16 pieces, 24 B per four values
    return (n_gsm + 4 * (size_t)H) * sizeof(float) + fused_small_bytes(e) + (zb + 2 * (size_t)C * NT * F_TILE) * sizeof(float);
}
// GPE_BWD_B6: the cooperative reverse kernel with its adjoint products on the bf16 pipe exists for plain MLPs of one to three maps at
// H <= 64; residual blocks and four / five maps keep the fp32 f_backward_coop
static bool coop_b6(const gpe_engine* e) {
    return e->bwd_b6 && e->H <= 64 && e->nd.n_lin - 2 <= 3 && e->cfg.net_kind == GPE_NET_MLP;
}
#define REV_ARGS e->nd, e->theta, e->WpkT, b.pts, b.stored, b.Ob, e->gslab, b.n, b.ld, e->Ppad      // what every fused reverse kernel takes first
// seeds: the pipelined kernel forms the seeds itself from these (mlp_backward's seeds_in_kernel); nullptr: they are in b.Ob already
template <int HH, int CC, int EE>
static void launch_f_backward_coop(gpe_engine* e, Batch& b, unsigned grid, size_t lds, const SeedArgs* seeds) {
    const int maps = e->nd.n_lin - 2;
    pick_n_out(e->nd.n_out, [&](auto no) {
        constexpr int NO = decltype(no)::value;
        if constexpr (HH <= 64) if (coop_b6(e)) {
            pick_int<1, 3>(maps, [&](auto nh) {
                hipLaunchKernelGGL((f_backward_coop<HH, CC, EE, NO, decltype(nh)::value, true>), dim3(grid), dim3(HH * 4), lds, e->stream, REV_ARGS);
            });
            return;
        }
        if constexpr (pipe_form(HH, CC)) if (use_pipe(e, CC)) {
            // small batch: the kernel forms the seeds itself (k_seed_pde was not launched); otherwise the large batches' uneven tile split
            const bool sd = seeds && head_form(HH, CC, NO);
            SeedArgs sa = sd ? *seeds : SeedArgs{};
            if (!sd) sa.old_share_q10 = pipe_tile_share(e, b, grid);
            pick_int<1, 3>(maps, [&](auto nh) { pick_int<0, 1>(sd, [&](auto s) {
                constexpr bool SEEDS = decltype(s)::value;
                if constexpr (!SEEDS || head_form(HH, CC, NO))
                    hipLaunchKernelGGL((f_backward_pipe<HH, CC, EE, NO, decltype(nh)::value, SEEDS>), dim3(grid), dim3(HH * 4), lds, e->stream, REV_ARGS, sa);
            }); });
            return;
        }
        const bool res = e->cfg.net_kind == GPE_NET_RESIDUAL && HH <= 64 && NO == 1;
        pick_int<1, 5>(res ? (maps == 2 ? 2 : 4) : maps, [&](auto nh) { pick_int<0, 1>(res, [&](auto r) {
            constexpr int NH = decltype(nh)::value;
            constexpr bool RES = decltype(r)::value;
            if constexpr (coop_form(HH, NO, NH, RES))
                hipLaunchKernelGGL((f_backward_coop<HH, CC, EE, NO, NH, false, RES>), dim3(grid), dim3(HH * 4), lds, e->stream, REV_ARGS);
        }); });
    });
}
template <int HH, int CC, int EE>
static void launch_f_backward(gpe_engine* e, Batch& b, unsigned grid, size_t lds, const SeedArgs* seeds) {
    const int kind = bwd_kind(e, b);
    if (kind == 3) return launch_f_backward_coop<HH, CC, EE>(e, b, grid, lds, seeds);
    // kind 2 (H <= 64): the weight gradients of one to three maps in registers, weights in LDS; kind 0: the plain kernel
    pick_n_out(e->nd.n_out, [&](auto no) { pick_int<0, 3>(kind == 2 ? e->nd.n_lin - 2 : 0, [&](auto nh) {
        constexpr int NO = decltype(no)::value, NH = decltype(nh)::value;
        if constexpr (NH == 0 || HH <= 64)
            hipLaunchKernelGGL((f_backward<HH, CC, EE, NO, (NH > 0), NH>), dim3(grid), dim3(256), lds, e->stream, REV_ARGS, e->nslab_g);
    }); });
}
#undef REV_ARGS

// persistent grids: forward 256-thread blocks, 2 per CU; reverse 256-thread x 2 per CU, or 512-thread x 1 per CU (WLDS)
static unsigned fused_grid(gpe_engine* e, int64_t n, int waves_per_block, int blocks_per_cu) {
    int64_t ntiles = (n + 15) / 16;
    int64_t blocks = (ntiles + waves_per_block - 1) / waves_per_block;
    int64_t cap = (int64_t)e->num_cu * blocks_per_cu;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

static size_t fused_bwd_lds(gpe_engine* e, int C, int kind) {
    if (e->H > 64) return ((size_t)4 * e->H + (size_t)4 * C * F_TILE) * sizeof(float) + fused_small_bytes(e);
    const int nwaves = 4;
    const bool w = kind != 0;
    return ((size_t)e->Ppad + 4 * (size_t)e->H + (size_t)nwaves * C * F_TILE) * sizeof(float) + fused_small_bytes(e) +
           (w ? fused_w_bytes(e) : 0);
}

// elements of a packed copy of the hidden-hidden weights (fused path; the generic set packs nothing)
static int pack_count(const gpe_engine* e) { return e->path == GPE_PATH_FUSED ? (e->nd.n_lin - 2) * e->H * e->H : 0; }

static int ensure_packed(gpe_engine* e) {
    if (e->path != GPE_PATH_FUSED || !e->packed_dirty) return GPE_OK;
    hipLaunchKernelGGL(k_pack_weights, dim3(cdiv(pack_count(e), 256)), dim3(256), 0, e->stream, e->nd, e->H, e->theta, e->Wpk,
                       e->WpkT);
    HIPCHK(e, hipGetLastError());
    e->packed_dirty = false;
    return GPE_OK;
}

// zero the step accumulators (+ repack weights when stale) in one launch
static int launch_begin(gpe_engine* e, bool force = false) {
    // fused path: k_update zeroed the sums and repacked the weights, and the first slab reduction assigns -> nothing to do
    if (!force && e->path == GPE_PATH_FUSED && e->acc_clean && !e->packed_dirty) { e->acc_clean = false; return GPE_OK; }
    e->acc_clean = false;
    const int n_pack = e->packed_dirty ? pack_count(e) : 0;
    const int n_dbl = DBL_COUNT, n_grad = e->P + GT_COUNT, n_bc = e->P;
    const int n = std::max(std::max(n_pack, n_dbl), n_grad);
    hipLaunchKernelGGL(k_begin, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, e->nd, e->H, e->theta, e->Wpk, e->WpkT, n_pack,
                       e->dbl, n_dbl, e->grad, n_grad, e->grad_bc, n_bc);
    HIPCHK(e, hipGetLastError());
    if (n_pack) e->packed_dirty = false;
    return GPE_OK;
}

static void prof_mark(gpe_engine* e, int kind, bool start) {
    if (!e->prof) return;
    if (start) {
        if (2 * e->ev_used + 1 >= e->ev_pool.size()) {
            hipEvent_t a, b2;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b2) != hipSuccess) return;
            e->ev_pool.push_back(a); e->ev_pool.push_back(b2); e->ev_kind.push_back(kind);
        } else e->ev_kind[e->ev_used] = kind;
        e->ev_used++;
    }
    if (e->ev_used == 0) return;
    size_t idx = e->ev_used - 1;
    (void)hipEventRecord(e->ev_pool[2 * idx + (start ? 0 : 1)], e->stream);
}

static WideCall wide_call(gpe_engine* e, Batch& b) {
    WideCall a;
    a.nd = e->nd; a.theta = e->theta; a.Wpk = e->Wpk; a.WpkT = e->WpkT; a.pts = b.pts; a.stored = b.stored; a.O = b.O; a.Ob = b.Ob;
    a.Z0 = b.Z0; a.Z1 = b.Z1; a.gslab = e->gslab; a.N = b.n; a.ld = b.ld; a.Ppad = e->Ppad; a.H = e->H; a.C = b.C; a.E = b.E;
    a.num_cu = e->num_cu; a.stream = e->stream;
    return a;
}

// frozen: the parameter set of a frozen orthogonality state instead of the trained one (its packed copies never go stale)
// head_slots > 0: the head rides in this pass, whose workgroups (that many) each leave a triple in e->head_slots (step_begin only)
static int mlp_forward(gpe_engine* e, Batch& b, bool store, const FwdWeights* frozen = nullptr, int head_slots = 0) {
    if (b.n <= 0) return GPE_OK;
    const bool mark = e->prof && (&b == &e->main);
    const FwdWeights W = frozen ? *frozen : FwdWeights{e->theta, e->Wpk, e->WpkT};
    if (e->path == GPE_PATH_FUSED) {
        int rc = frozen ? GPE_OK : ensure_packed(e);
        if (rc) return rc;
        if (mark) prof_mark(e, 0, true);
        if (e->wide_fwd) {
            WideCall wc = wide_call(e, b);
            wc.theta = W.theta; wc.Wpk = W.Wpk; wc.WpkT = W.WpkT;
            const int wr = wide_forward(wc, store ? 1 : 0);
            if (wr < 0) FAIL(e, GPE_ERR_INVALID, "wide kernel set: channels (%d,%d) / n_out %d not compiled", b.C, b.E, e->nd.n_out);
            if (wr) FAIL(e, GPE_ERR_HIP, "w_forward launch: %s", hipGetErrorString((hipError_t)wr));
            if (mark) prof_mark(e, 0, false);
            return GPE_OK;
        }
        // H = 128 (wide layers): C <= 5, dim <= 2 (checked at create)
        if ((rc = launch_hce<ce_forward, ce_h128_forward>(e, b, [&](auto HH, auto CC, auto EE) { launch_f_forward<HH, CC, EE>(e, b, store ? 1 : 0, W, head_slots > 0); }))) return rc;
        if (mark) prof_mark(e, 0, false);
    } else {
        const NetDesc& nd = e->nd;
        for (int lin = 0; lin < nd.n_lin; ++lin) {
            const float* Sprev = lin > 0 ? b.S[lin - 1] : nullptr;
            float* Out = (lin == nd.n_lin - 1) ? b.O : b.S[lin];
            const float* Sskip = nd.skip[lin] >= 0 ? b.S[nd.skip[lin]] : nullptr;     // residual block: the VALU kernel adds the block input
            if (!Sskip && lin > 0 && nd.width[lin] % 64 == 0 && nd.width[lin + 1] % 256 == 0 && e->gen_mfma && e->gen_mfma2) {
                dim3 grid(cdiv(b.n, 16), nd.width[lin + 1] / 256);      // a block = one point tile x 256 outputs, jets shared through LDS
                if (int rc = launch_ce(e, b, ce_forward{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_fwd_layer_mfma2<CC, EE>), grid, dim3(256), 0, e->stream, nd, lin, W.theta,
                                                    Sprev, Out, b.n, b.ld); })) return rc;
            } else if (lin > 0 && nd.width[lin] % 64 == 0 && nd.width[lin + 1] % 64 == 0 && e->gen_mfma &&
                       (!Sskip || nd.width[nd.skip[lin] + 1] == nd.width[lin + 1])) {   // wide map: matrix cores (round 4: residual blocks too)
                dim3 grid(cdiv(cdiv(b.n, 16), 4), nd.width[lin + 1] / 64);
                if (int rc = launch_ce(e, b, ce_forward{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_fwd_layer_mfma<CC, EE>), grid, dim3(256), 0, e->stream, nd, lin, W.theta,
                                                    Sprev, Out, b.n, b.ld, Sskip); })) return rc;
            } else if (nd.width[lin + 1] >= 64) {      // wide layer: 16 output features per thread
                dim3 grid(cdiv(b.n, 256), cdiv(nd.width[lin + 1], G_FBW));
                if (int rc = launch_ce(e, b, ce_forward{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_fwd_layer<CC, EE, G_FBW>), grid, dim3(256), 0, e->stream, nd, lin, W.theta,
                                                    b.pts, Sprev, Out, b.n, b.ld, Sskip); })) return rc;
            } else {
                dim3 grid(cdiv(b.n, 256), cdiv(nd.width[lin + 1], G_FB));
                if (int rc = launch_ce(e, b, ce_forward{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_fwd_layer<CC, EE, G_FB>), grid, dim3(256), 0, e->stream, nd, lin, W.theta,
                                                    b.pts, Sprev, Out, b.n, b.ld, Sskip); })) return rc;
            }
        }
    }
    HIPCHK(e, hipGetLastError());
    return GPE_OK;
}

static int bc_join(gpe_engine* e);
static double bc_count(gpe_engine* e);
static int launch_tail(gpe_engine* e, bool add_bc);
static int dp_allreduce(gpe_engine* e, void* buf, size_t count, ncclDataType_t dt, hipEvent_t behind);
// pack_mode of the single-workgroup update (update_core): 1 gather pass, 2 scatter in the Adam loop; bits 0 and 2: GPE_UPDATE_CACHE=0
static int update_pack_mode(const gpe_engine* e) { return ((e->fwd_b6 || e->bwd_b6 || e->H > 64) ? 1 : 2) | (e->update_cache ? 0 : 5); }
// whole steps on small parameter vectors: the slab reduction that closes the step runs the update itself (k_reduce_update) ...
static bool reduce_runs_update(const gpe_engine* e, const BwdOpts& o) {
    return o.close && o.assign && o.update_may_fuse && e->fuse_update && e->upd_ticket && !e->upd_snap && e->update_cache && e->P <= UPD_REG_E * 1024 && !e->dp.on();
}
// ... or leaves partial norms and the snapshot for the update on UPD_G workgroups (k_grad_reduce_part)
static bool reduce_leaves_parts(const gpe_engine* e, const BwdOpts& o) {
    return o.close && o.assign && o.update_may_fuse && e->split_update && e->upd_snap_small && !e->upd_snap && !e->dp.on() && !e->ext_exchange &&
           !e->fwd_b6 && !e->bwd_b6 && e->H <= 64;
}
// Gradient of one batch into e->grad: assigned (first reverse pass of the step) or accumulated.  o.close: this is the last reverse pass of the step -- join the boundary batch's side stream, add its
// gradient and write the exchange tail (folded into the slab reduction on the fused path)
static int mlp_backward(gpe_engine* e, Batch& b, const BwdOpts& o) {
    const bool close = o.close, assign = o.assign;
    if (b.n <= 0) return close ? launch_tail(e, true) : GPE_OK;
    if (e->path == GPE_PATH_FUSED) {
        // the seeds the kernel forms add the head triples this step's forward pass left, if it ran the head
        const SeedArgs sa{e->ph, b.V, b.u, b.Hu, (const double*)e->sums(), e->dsc(), e->n_pde, e->st.head_slots ? (const double*)e->head_slots : nullptr,
                          e->st.head_slots, e->sums(), e->lsums(), 0};
        const SeedArgs* seeds = o.seeds_in_kernel ? &sa : nullptr;
        const int kind = bwd_kind(e, b);
        unsigned grid = kind == 3 ? fused_grid(e, b.n, 1, e->coop_wg_per_cu)
                                  : (kind == 2 ? fused_grid(e, b.n, 4, 1) : fused_grid(e, b.n, 4, 2));
        size_t lds = kind == 3 ? coop_lds(e, b.C) : fused_bwd_lds(e, b.C, kind);
        const bool mark = e->prof && (&b == &e->main);
        if (mark) prof_mark(e, 1, true);
        int nred = (int)grid;
        if (wide_reverse(e, b)) {
            if (!b.Z0) FAIL(e, GPE_ERR_STATE, "reverse pass on a forward-only batch");
            const int wr = wide_backward(wide_call(e, b));
            if (wr < 0) FAIL(e, GPE_ERR_INVALID, "wide kernel set: channels (%d,%d) / n_out %d not compiled", b.C, b.E, e->nd.n_out);
            if (wr) FAIL(e, GPE_ERR_HIP, "wide reverse launch: %s", hipGetErrorString((hipError_t)wr));
            nred = wide_groups(e->H, b.n, e->num_cu);
        } else {
        if (e->H == 128) {      // one workgroup per CU; the plain kernel adds into global slabs
            grid = fused_grid(e, b.n, kind == 3 ? 1 : 4, 1);
            nred = kind == 3 ? (int)grid : e->nslab_g;
            if (kind != 3) HIPCHK(e, hipMemsetAsync(e->gslab, 0, (size_t)e->nslab_g * e->Ppad * sizeof(float), e->stream));
        }
        const int rc = launch_hce<ce_train, ce_h128_reverse>(e, b, [&](auto HH, auto CC, auto EE) { launch_f_backward<HH, CC, EE>(e, b, grid, lds, seeds); });
        if (rc) return rc;
        }
        if (mark) prof_mark(e, 1, false);
        HIPCHK(e, hipGetLastError());
        const float* add = nullptr;
        if (close) {
            int rc = bc_join(e);
            if (rc) return rc;
            if (e->st.bc_inflight) add = e->grad_bc;
            e->st.bc_inflight = false;
        }
        if (reduce_runs_update(e, o)) {
            hipLaunchKernelGGL(k_reduce_update, dim3(cdiv(e->P, 64)), dim3(1024), 0, e->stream, e->gslab, nred, e->Ppad, e->P, e->grad, add,
                               (const double*)e->dsc(), e->upd_ticket, e->theta, e->am, e->av, (const double*)e->sums(), (const double*)e->lsums(),
                               e->ph, e->oc, e->od, e->hist, e->cap, e->last, bc_count(e), e->nd, e->H, e->Wpk, e->WpkT, pack_count(e), e->dbl,
                               (int)DBL_COUNT, update_pack_mode(e));
            e->st.update_done = true;
        } else if (reduce_leaves_parts(e, o)) {
            hipLaunchKernelGGL(k_grad_reduce_part, dim3(UPD_G), dim3(1024), 0, e->stream, e->gslab, nred, e->Ppad, e->P, e->grad, add,
                               (const double*)e->dsc(), (const double*)e->sums(), (const double*)e->lsums(), (const OptDev*)e->od, e->upd_snap_small);
            e->st.update_parts = true;
        } else
        hipLaunchKernelGGL(k_grad_reduce, dim3(cdiv(e->P, 64)), dim3(1024), 0, e->stream, e->gslab, nred, e->Ppad,
                           e->P, e->grad, add, close ? (const double*)e->dsc() : (const double*)nullptr, assign ? 1 : 0);
    } else {
        const NetDesc& nd = e->nd;
        float* Zb = b.Ob;
        float* nxt = b.A0;
        const float* skip_adj = nullptr;          // zbar of a residual block's second map: joins the adjoint of the block input
        int skip_to = -1;
        for (int lin = nd.n_lin - 1; lin >= 0; --lin) {
            const int K = nd.width[lin], Ho = nd.width[lin + 1];
            const float* Sprev = lin > 0 ? b.S[lin - 1] : nullptr;
            if (nd.skip[lin] >= 0) { skip_adj = Zb; skip_to = nd.skip[lin]; }
            if (lin > 0 && Ho % 128 == 0 && K % 128 == 0 && e->gen_mfma && e->gen_mfma2) {
                // wide hidden->hidden map, 128 x 128 block tiles with LDS-shared operand panels
                const int64_t want = (int64_t)e->num_cu * 4 / ((Ho / 128) * (K / 128)) + 1;       // ~4 blocks per CU
                int64_t chunk = ((b.n + want - 1) / want + 15) / 16 * 16;
                if (chunk < 256) chunk = 256;
                const int64_t nchunk = (b.n + chunk - 1) / chunk;
                dim3 gw(Ho / 128, K / 128, (unsigned)nchunk);
                const size_t pl = (size_t)2 * b.C * 128 * 16 * sizeof(float);
                if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_bwd_weight_mfma2<CC, EE>), gw, dim3(256), pl, e->stream, nd, lin, Sprev, Zb,
                                                    e->grad, b.n, b.ld, chunk); })) return rc;
            } else if (lin > 0 && Ho % 64 == 0 && K % 64 == 0 && e->gen_mfma) {
                // wide hidden->hidden map: split-K GEMM over the points on the matrix cores
                const int64_t want = (int64_t)e->num_cu * 16 / ((Ho / 64) * (K / 64)) + 1;          // chunks so that ~16 waves per CU exist
                int64_t chunk = ((b.n + want - 1) / want + 15) / 16 * 16;
                // (a 64 x 64 map over 4 000 points -- the residual network of refine/box_to_gaussian at its own size -- ran as 16 waves of
                // 256 points each, 100 us per map; measured per step at 256 / 128 / 64 / 32 points per wave: 637 / 447 / 348 / 312 us -- the atomics of a
                // 64 x 64 block cost less than the serial walk)
                if (chunk < e->gen_min_chunk) chunk = e->gen_min_chunk;
                const int64_t nchunk = (b.n + chunk - 1) / chunk;
                dim3 gw(Ho / 64, K / 64, (unsigned)((nchunk + 3) / 4));
                if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_bwd_weight_mfma<CC, EE>), gw, dim3(256), 0, e->stream, nd, lin, Sprev, Zb,
                                                    e->grad, b.n, b.ld, chunk); })) return rc;
            } else if (Ho >= 64 && K >= 16) {   // wide layer: 8 rows of the weight gradient per block share the recomputed jets
                dim3 gw(cdiv(Ho, 8), cdiv(K, G_KB));
                if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_bwd_weight<CC, EE, 8, G_KB>), gw, dim3(256), 0, e->stream, nd, lin, b.pts, Sprev,
                                                    Zb, e->grad, b.n, b.ld); })) return rc;
            } else if (Ho < 8 && K >= 64) {     // output layer of a wide network: one block per (n, k) keeps K blocks in flight
                dim3 gw(Ho, K);
                if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_bwd_weight<CC, EE, 1, 1>), gw, dim3(256), 0, e->stream, nd, lin, b.pts, Sprev,
                                                    Zb, e->grad, b.n, b.ld); })) return rc;
            } else {
                dim3 gw(Ho, cdiv(K, G_KB));
                if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_bwd_weight<CC, EE, 1, G_KB>), gw, dim3(256), 0, e->stream, nd, lin, b.pts, Sprev,
                                                    Zb, e->grad, b.n, b.ld); })) return rc;
            }
            if (o.bucketed && close) {
                // data-parallel step: this map's gradient slice (weights + bias, contiguous) is final -> all-reduce it on the
                // exchange stream behind the remaining reverse pass (output map first)
                int rcb = dp_allreduce(e, e->grad + nd.offW[lin], (size_t)K * Ho + Ho, ncclFloat, e->dp.ev_bucket[lin]);
                if (rcb) return rcb;
            }
            if (lin > 0) {
                bool act_done = false;
                const bool join = skip_adj && skip_to == lin - 1;      // the skipped-from layer: its adjoint gets the saved zbar first
                if (!join && K % 256 == 0 && Ho % 64 == 0 && e->gen_mfma && e->gen_mfma2) {
                    dim3 gd(cdiv(b.n, 16), K / 256);             // activation adjoint of layer lin-1 fused into the epilogue
                    if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_bwd_data_mfma2<CC, EE>), gd, dim3(256), 0, e->stream, nd, lin, e->theta, Zb,
                                                        nxt, Sprev, b.n, b.ld); })) return rc;
                    act_done = true;
                } else if (K % 64 == 0 && Ho % 16 == 0 && e->gen_mfma) {
                    dim3 gd(cdiv(cdiv(b.n, 16), 4), K / 64);
                    if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_bwd_data_mfma<CC>), gd, dim3(256), 0, e->stream, nd, lin, e->theta, Zb,
                                                        nxt, b.n, b.ld); })) return rc;
                } else if (K >= 64) {
                    dim3 gd(cdiv(b.n, 256), cdiv(K, G_FBW));
                    if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_bwd_data<CC, G_FBW>), gd, dim3(256), 0, e->stream, nd, lin, e->theta, Zb,
                                                        nxt, b.n, b.ld); })) return rc;
                } else {
                    dim3 gd(cdiv(b.n, 256), cdiv(K, G_FB));
                    if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_bwd_data<CC, G_FB>), gd, dim3(256), 0, e->stream, nd, lin, e->theta, Zb,
                                                        nxt, b.n, b.ld); })) return rc;
                }
                if (join) {
                    const int64_t cnt = (int64_t)b.C * K * b.ld;
                    hipLaunchKernelGGL(g_add, dim3(cdiv(cnt, 256)), dim3(256), 0, e->stream, nxt, skip_adj, cnt);
                    skip_adj = nullptr; skip_to = -1;
                }
                if (!act_done) {
                    dim3 ga(cdiv(b.n, 256), K);
                    if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((g_bwd_act<CC, EE>), ga, dim3(256), 0, e->stream, K, Sprev, nxt, b.n, b.ld); })) return rc;
                }
                Zb = nxt;
                // next free adjoint buffer: not the one just written, not one still waiting for its skip join
                float* cand[3] = {b.A0, b.A1, b.A2};
                for (float* c2 : cand) if (c2 && c2 != Zb && c2 != skip_adj) { nxt = c2; break; }
            }
        }
        if (close) {
            int rc = bc_join(e);
            if (rc) return rc;
            if ((rc = launch_tail(e, true))) return rc;
        }
    }
    HIPCHK(e, hipGetLastError());
    return GPE_OK;
}

// ---- config -> device structs ------------------------------------------------------------------------
// N of the means without quadrature weights: the configured global count, or the bound local one
static double counted_n_global(const gpe_engine* e) {
    return (double)(e->cfg.n_global > 0 ? e->cfg.n_global : (e->n_pde > 0 ? e->n_pde : 1));
}
static void fill_phys(gpe_engine* e) {
    const gpe_config& c = e->cfg;
    Phys& p = e->ph;
    memset(&p, 0, sizeof p);
    p.dim = c.layers[0]; p.n_out = c.layers[c.n_layers - 1]; p.complex_psi = c.complex_psi;
    p.kin = c.kinetic_coeff; p.potential = c.potential; p.pot_scale = c.pot_scale;
    for (int k = 0; k < 3; ++k) p.omega[k] = c.omega[k];
    p.pot_a = c.pot_a; p.pot_v0 = c.pot_v0; p.pot_k = c.pot_k; p.omega_rot = c.omega_rot;
    p.gamma = c.gamma; p.p = c.p; p.abs_power = c.abs_power; p.base_mode = c.base_mode; p.base_deriv = c.base_deriv;
    p.base_kind = c.base_kind; p.envelope = c.envelope; p.box_L = c.box_L > 0.f ? c.box_L : 1.f; p.env_L = c.env_L > 0.f ? c.env_L : 1.f;
    p.perturb_scale = c.perturb_scale; p.bc_nn_scale = c.bc_nn_scale;
    p.w_pde = c.w_pde; p.w_bc = c.w_bc; p.w_norm = c.w_norm; p.w_sym = c.w_sym; p.w_orth = c.w_orth;
    p.sym_sign = c.sym_sign; p.dx = c.dx; p.w_riesz = c.w_riesz; p.riesz_kind = c.riesz_kind;
    p.lambda_kind = c.lambda_kind; p.w_reg_f = c.w_reg_f; p.reg_f_eps = c.reg_f_eps; p.w_reg_lam = c.w_reg_lam; p.reg_lam_eps = c.reg_lam_eps;
    p.n_global = e->wq ? e->wq_total : counted_n_global(e);        // bound weights: W = sum q over all ranks
    p.inv_world = 1.0f / (float)(c.world_size > 0 ? c.world_size : 1);
    int no = 0;
    for (int j = 0; j < GPE_MAX_ORTH; ++j) if (e->orth_host[j]) no = j + 1;      // [4..6] are the precomputed base
    p.n_orth = no;
    if (c.base_mode >= 0) {
        double f = 1.0;
        for (int i = 2; i <= c.base_mode; ++i) f *= i;
        e->base_norm = (float)pow(pow(2.0, c.base_mode) * f * sqrt(M_PI), -0.5);
    }
    OptCfg& o = e->oc;
    o.beta1 = c.beta1; o.beta2 = c.beta2; o.eps = c.eps; o.clip_norm = c.clip_norm; o.sched = c.sched;
    o.T_0 = c.T_0; o.T_mult = c.T_mult; o.eta_min = c.eta_min; o.factor = c.factor; o.patience = c.patience;
    o.min_lr = c.min_lr; o.threshold = c.threshold;
    o.stop_tol = c.stop_tol; o.stop_patience = c.stop_patience;
    MixPhys& mx = o.mix;
    mx.on = c.mixture != 0;
    for (int k = 0; k < 3; ++k) mx.g[k] = c.mixture ? c.mix_g[k] : 0.f;
    for (int k = 0; k < 2; ++k) mx.n[k] = c.mixture ? c.mix_norm[k] : 0.f;
    mx.wE = c.mixture ? e->mix_wE : 0.f;
}

// device-resident L-BFGS (gpe_lbfgs.h): its state is reset with the optimiser and whenever the parameters are replaced
// theta_to_start: the caller does not rewrite theta, so a running line search is ended by putting theta back to its start point
static int lbfgs_reset(gpe_engine* e, bool theta_to_start = false) {
    if (!e->lb.st) return GPE_OK;
    if (theta_to_start && e->lb.ls.kind && e->lb.ls_buf) {
        hipLaunchKernelGGL(k_ls_restore, dim3(cdiv(e->P, 256)), dim3(256), 0, e->stream, e->P, e->theta, (const LbfgsDev*)e->lb.st);
        HIPCHK(e, hipGetLastError());
        e->packed_dirty = true;
    }
    LbfgsDev h;
    memset(&h, 0, sizeof h);
    h.H_diag = 1.0; h.prev_loss = INFINITY;
    if (e->lb.ls_buf) { h.ls.slots = e->lb.ls_buf; h.ls.theta0 = e->lb.ls_buf + (size_t)LS_SLOTS * e->lb.ld; }
    HIPCHK(e, hipMemcpyAsync(e->lb.st, &h, sizeof h, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

static void lbfgs_free_history(gpe_engine* e) {
    gpe_engine::Lbfgs::Hist& h = e->lb.h;
    void* ps[] = {h.S, h.Y, h.g_prev, h.d, h.part, h.SY, h.YY, h.ro, h.coef};
    for (void* p : ps) if (p) (void)hipFree(p);
    h = gpe_engine::Lbfgs::Hist();
}

static void lbfgs_free(gpe_engine* e) {
    lbfgs_free_history(e);
    void* ps[] = {e->lb.st, e->lb.ls_buf, e->lb.ls_part, e->lb.view_buf};
    for (void* p : ps) if (p) (void)hipFree(p);
    e->lb = gpe_engine::Lbfgs();
}

static int reset_opt(gpe_engine* e, float lr) {
    OptDev h;
    memset(&h, 0, sizeof h);
    h.lr = lr; h.lr0 = lr; h.best = INFINITY; h.num_bad = 0; h.nonfinite = 0; h.step = 0;
    h.stopped = 0; h.es_count = 0; h.es_best = INFINITY; h.stop_step = 0; h.b1p = 1.0; h.b2p = 1.0;
    HIPCHK(e, hipMemcpyAsync(e->od, &h, sizeof h, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemsetAsync(e->am, 0, (size_t)e->P * sizeof(float), e->stream));
    HIPCHK(e, hipMemsetAsync(e->av, 0, (size_t)e->P * sizeof(float), e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return lbfgs_reset(e, /*theta_to_start=*/true);
}

// ---- engine creation, phase by phase (gpe_create calls each once, in this order) -------------------------------------------------------
// check_config, pad_widths, describe_net and select_path work on the configuration alone: no HIP call, so every refusal comes before the
// device is touched.  The first rule that fails is the one the caller sees.
#define CFAIL(...) do { char _b[512]; snprintf(_b, sizeof _b, __VA_ARGS__); e->err = _b; return GPE_ERR_INVALID; } while (0)
// 1. every refusal that needs the configuration only
static int check_config(gpe_engine* e, const gpe_config& in) {
    if (in.abi_version != GPE_ABI_VERSION) CFAIL("abi_version %d != %d", in.abi_version, GPE_ABI_VERSION);
    const gpe_config& c = e->cfg = in;
    e->obs_kind = c.mixture ? &OBS_MIXTURE : &OBS_SCALAR;
    if (c.n_layers < 3 || c.n_layers > GPE_MAX_LAYERS) CFAIL("n_layers must be in [3,%d]", GPE_MAX_LAYERS);
    const int dim = c.layers[0], no = c.layers[c.n_layers - 1];
    if (dim < 1 || dim > GPE_MAX_DIM) CFAIL("dim must be 1..3");
    if (no < 1 || no > 2) CFAIL("output width must be 1 or 2");
    if (c.mixture) {                  // two real components on the n_out = 2 kernels: what does not combine with them, first failing rule first
        if (no != 2 || c.p != 3) CFAIL("a mixture needs out=2 and p=3");
        if (c.complex_psi) CFAIL("a mixture has two real components: complex psi does not combine with it");
        if (c.omega_rot != 0.f) CFAIL("a mixture has no rotating frame: omega_rot must be 0");
        if (c.base_mode >= 0) CFAIL("a mixture has no analytic base: base_mode must be -1");
        if (c.envelope != GPE_ENV_NONE) CFAIL("a mixture has no boundary factor: envelope must be GPE_ENV_NONE");
        if (c.w_sym != 0.f) CFAIL("a mixture has no symmetry term: w_sym must be 0");
        if (c.w_orth != 0.f) CFAIL("a mixture has no orthogonality term: w_orth must be 0");
        if (c.w_riesz != 0.f) CFAIL("a mixture has no Riesz energy term: w_riesz must be 0");
        if (c.lambda_kind != GPE_LAMBDA_RAYLEIGH) CFAIL("a mixture takes one Rayleigh quotient per component: lambda_kind must be GPE_LAMBDA_RAYLEIGH");
        if (c.w_reg_f != 0.f || c.w_reg_lam != 0.f) CFAIL("a mixture has no regularisers: w_reg_f and w_reg_lam must be 0");
        if (c.net_kind != GPE_NET_MLP) CFAIL("a mixture needs a plain MLP: residual blocks do not combine with it");
        for (int k = 0; k < 3; ++k) if (!__builtin_isfinite(c.mix_g[k])) CFAIL("mixture coupling mix_g[%d] is not finite", k);
        for (int k = 0; k < 2; ++k) if (!(c.mix_norm[k] > 0.f) || !__builtin_isfinite(c.mix_norm[k])) CFAIL("mixture target norm mix_norm[%d] must be finite and > 0", k);
    }
    if (c.complex_psi && (no != 2 || c.p != 3)) CFAIL("complex psi needs out=2 and p=3");
    if (!c.complex_psi && !c.mixture && no != 1) CFAIL("real psi needs out=1");
    if (c.potential < 0 || c.potential > GPE_POT_NONE) CFAIL("Unknown potential type: %d", c.potential);
    if (c.base_mode >= 0 && (dim != 1 || no != 1)) CFAIL("Hermite base needs dim=1, out=1");
    if (c.p < 1 || c.p > 32) CFAIL("power p must be in [1,32]");
    if (c.omega_rot != 0.f && (!c.complex_psi || dim < 2)) CFAIL("rotation needs complex psi and dim>=2");
    if (c.base_kind < 0 || c.base_kind > GPE_BASE_PRECOMPUTED) CFAIL("Unknown base kind: %d", c.base_kind);
    if (c.envelope < 0 || c.envelope > GPE_ENV_SIN) CFAIL("Unknown envelope: %d", c.envelope);
    if (c.envelope != GPE_ENV_NONE && (dim != 1 || no != 1)) CFAIL("the boundary factor needs dim=1, out=1");
    if (c.w_riesz != 0.f && no != 1 && !(c.complex_psi && no == 2 && c.p == 3))
        CFAIL("the Riesz energy term needs real psi (out=1) or complex psi (out=2) with p = 3");
    if (c.riesz_kind < 0 || c.riesz_kind > GPE_RIESZ_VARIATIONAL) CFAIL("Unknown Riesz kind: %d", c.riesz_kind);
    if (c.lambda_kind != GPE_LAMBDA_RAYLEIGH && c.lambda_kind != GPE_LAMBDA_ENERGY) CFAIL("Unknown lambda kind: %d", c.lambda_kind);
    if (c.lambda_kind == GPE_LAMBDA_ENERGY && (c.complex_psi || no != 1 || (c.p & 1) == 0))
        CFAIL("the energy-functional lambda needs real psi (out=1) and an odd power p");
    if (c.w_reg_lam != 0.f && c.lambda_kind != GPE_LAMBDA_ENERGY) CFAIL("the 1/lambda^2 regulariser needs the energy-functional lambda");
    if ((c.w_reg_f != 0.f || c.w_reg_lam != 0.f) && (c.complex_psi || no != 1)) CFAIL("the regularisers need real psi (out=1)");
    if ((c.w_reg_f != 0.f && !(c.reg_f_eps > 0.f)) || (c.w_reg_lam != 0.f && !(c.reg_lam_eps > 0.f))) CFAIL("regulariser eps must be > 0");
    for (int i = 1; i < c.n_layers - 1; ++i)
        if (c.layers[i] < 1 || c.layers[i] > 1024) CFAIL("hidden width %d out of range", c.layers[i]);
    return GPE_OK;
}

// the whole-network kernels at H <= 64 keep all parameters (padded to 64) in LDS: the one rule pad_widths picks a width by and select_path
// admits a network to the fused set by
static bool fused_lds_fits(size_t Ppad, int n_lin, int H, int dim) {
    return (Ppad + (size_t)(8 + n_lin + 3) * H + 8 + 4 * (dim + 2) * F_TILE) * sizeof(float) <= 160 * 1024;
}

// 2. Width padding.  The MFMA kernel sets are instantiated for one hidden width of 32, 64, 128 or 256; other plain-tanh MLPs of width <= 256 --
// the 2D scripts' own [2,100,100,100,1] (src/gross_pitaevskii_2D_minimal.py:377), ragged widths -- are run as the next such width with
// zero rows / columns / biases in the padding.  A padded unit sees z = 0, gives tanh(0) = 0 with all jets 0, feeds zero outgoing weights
// and so receives the gradient 0 exactly on every one of its weights: Adam leaves them at 0 and the network stays the caller's.
// ShiftedTanh (tanh + 1) would give 1 there: its padded units get the bias -40 instead of 0 -- tanh(-40) = -1 exactly in fp32 (exp(-80) + 1 = 1),
// so the unit outputs exactly 0 with slope 1 - t^2 = 0, every gradient that touches it is 0 again, and the bias itself stays where it is.
// GPE_PAD_WIDTH=0 or GPE_PATH_GENERIC: as given.  Fills user_layers, and for a padded network umap, pad_bias, P_user and the padded cfg.layers.
static void pad_widths(gpe_engine* e) {
    const gpe_config& c = e->cfg;
    const int dim = c.layers[0], no = c.layers[c.n_layers - 1];
    for (int i = 0; i < c.n_layers; ++i) e->user_layers[i] = c.layers[i];
    int wmax = 0; bool uni = true;
    for (int i = 1; i < c.n_layers - 1; ++i) { wmax = std::max(wmax, c.layers[i]); uni = uni && c.layers[i] == c.layers[1]; }
    const bool native = uni && (wmax == 32 || wmax == 64 || wmax == 128 || wmax == 256);
    // (widths above 256 -- train_pinn's default [2,400,400,400,1], src/gross_pitaevskii_2D_minimal.py:278 -- have no whole-network kernel: they are
    // padded to the next multiple of 256 so that the GENERIC set runs every hidden map on its 128 x 128-tile MFMA kernels instead of the VALU ones)
    const bool big = wmax > 256 && wmax <= 1024 && !(uni && wmax % 256 == 0);
    if (!(env_on("GPE_PAD_WIDTH") && (big || (!native && wmax <= 256)) && c.path != GPE_PATH_GENERIC && c.net_kind == GPE_NET_MLP &&
          (c.activation == GPE_ACT_TANH || c.activation == GPE_ACT_TANH_PLUS1) && c.n_layers - 2 >= 2))
        return;
    // the smallest instantiated width that holds the widest layer and whose kernels take this depth (32 / 64: all weights in LDS)
    int Hp = big ? (int)round_up(wmax, 256) : 0;
    if (!big)
    for (int h : {32, 64, 128, 256}) {
        if (h < wmax) continue;
        if (h <= 64) {
            const int Lm = c.n_layers - 3;                        // hidden -> hidden maps
            const size_t pp = round_up((size_t)dim * h + h + (size_t)Lm * (h * h + h) + (size_t)h * no + no, 64);
            if (!fused_lds_fits(pp, c.n_layers - 1, h, dim)) continue;
        }
        Hp = h; break;
    }
    int pl[GPE_MAX_LAYERS];
    for (int i = 0; i < c.n_layers; ++i) pl[i] = (i == 0 || i == c.n_layers - 1) ? c.layers[i] : Hp;
    int offp = 0;
    for (int j = 0; j + 1 < c.n_layers; ++j) {
        const int iu = c.layers[j], ou = c.layers[j + 1], ip = pl[j], op = pl[j + 1];
        for (int o = 0; o < ou; ++o) for (int i = 0; i < iu; ++i) e->umap.push_back(offp + o * ip + i);
        offp += ip * op;
        for (int o = 0; o < ou; ++o) e->umap.push_back(offp + o);
        if (c.activation == GPE_ACT_TANH_PLUS1 && j + 2 < c.n_layers) for (int o = ou; o < op; ++o) e->pad_bias.push_back(offp + o);
        offp += op;
    }
    e->P_user = (int)e->umap.size();
    for (int i = 1; i < c.n_layers - 1; ++i) e->cfg.layers[i] = Hp;
}

// 3. the network as the kernels see it: NetDesc, P, Ppad (and P_user of a network that runs as given)
static int describe_net(gpe_engine* e) {
    const gpe_config& c = e->cfg;
    const int dim = c.layers[0], no = c.layers[c.n_layers - 1];
    NetDesc& nd = e->nd;
    memset(&nd, 0, sizeof nd);
    nd.dim = dim; nd.n_out = no; nd.shift = c.activation == GPE_ACT_TANH_PLUS1 ? 1.f : 0.f;
    if (c.net_kind != GPE_NET_MLP && c.net_kind != GPE_NET_RESIDUAL) CFAIL("Unknown network kind: %d", c.net_kind);
    for (int j = 0; j < GPE_MAX_LAYERS; ++j) { nd.skip[j] = -1; nd.shiftv[j] = nd.shift; }
    if (c.net_kind == GPE_NET_RESIDUAL) {      // refine/box_to_gaussian_pinn_simulation.py:100-130
        const int nb = c.n_layers - 3;
        if (nb < 1 || 2 * nb + 3 > GPE_MAX_LAYERS) CFAIL("residual network: 1..%d blocks", (GPE_MAX_LAYERS - 3) / 2);
        for (int i = 2; i < c.n_layers - 1; ++i) if (c.layers[i] != c.layers[1]) CFAIL("residual network: one hidden width");
        nd.n_lin = 2 * nb + 2;
        nd.width[0] = dim;
        for (int i = 1; i <= 2 * nb + 1; ++i) nd.width[i] = c.layers[1];
        nd.width[nd.n_lin] = no;
        for (int bq = 0; bq < nb; ++bq) nd.skip[2 * bq + 2] = 2 * bq;     // lin2 of block bq adds hidden layer 2 bq (the block input)
        for (int h = 1; h < nd.n_lin - 1; ++h) nd.shiftv[h] = 0.f;        // plain tanh inside the blocks; the first layer keeps `activation`
    } else {
        nd.n_lin = c.n_layers - 1;
        for (int i = 0; i < c.n_layers; ++i) nd.width[i] = c.layers[i];
    }
    int off = 0;
    for (int j = 0; j < nd.n_lin; ++j) {
        nd.offW[j] = off; off += nd.width[j] * nd.width[j + 1];
        nd.offB[j] = off; off += nd.width[j + 1];
    }
    nd.n_params = off;
    e->P = off;
    if (e->umap.empty()) e->P_user = off;
    e->Ppad = (int)round_up(off, 64);
    return GPE_OK;
}

// 4. path and kernel set: path, H, wide, wide_fwd (and fwd_wg_per_cu, refused here when this build cannot honour it).
// The fused kernels need >= 2 hidden layers of one width H.  All of this is FIXED before read_switches parses GPE_COOP and the rest: a
// residual network admitted to the fused set here has only the cooperative <..., RES> kernels, and GPE_COOP=0 cannot take that back.
// Hence coop_only(): fwd_coop() / bwd_kind() ask it before they look at e->coop (such a network once ran the plain-MLP kernels: a silently wrong loss).
static int select_path(gpe_engine* e) {
    const gpe_config& c = e->cfg;
    const NetDesc& nd = e->nd;
    const int dim = nd.dim, no = nd.n_out, H = c.layers[1];
    bool uniform = true;
    for (int i = 2; i < c.n_layers - 1; ++i) uniform = uniform && (c.layers[i] == c.layers[1]);
    const int Lh = nd.n_lin - 1;                                                 // hidden layers (an MLP's n_layers - 2; a residual network's 2 blocks + 1)
    // residual blocks (refine/box_to_gaussian_pinn_simulation.py): round 4 -- one or two blocks of width 32 / 64, real psi, on the cooperative
    // whole-network kernels (f_forward_coop / f_backward_coop <..., RES>); everything else on the generic set
    const bool residual = c.net_kind == GPE_NET_RESIDUAL;
    if (residual && !((H == 32 || H == 64) && no == 1 && (nd.n_lin - 2 == 2 || nd.n_lin - 2 == 4))) uniform = false;
    if (residual && !env_on("GPE_RES_FUSED")) uniform = false;
    bool fused_ok = uniform && (H == 32 || H == 64) && Lh >= 2 && fused_lds_fits((size_t)e->Ppad, nd.n_lin, H, dim);
    if (residual && (H == 128 || H == 256)) uniform = false;                    // (no residual form of the 8-wave kernels)
    if (uniform && H == 128 && Lh >= 2 && dim <= 2) fused_ok = true;          // cooperative kernels, weights streamed from L2
    // wide kernel set: H = 256 and 3D H = 128 entirely; 1D/2D H = 128: its per-map reverse kernels (no register spills, -5..7 % against
    // f_backward_coop<128>) behind the cooperative forward kernel (7 % faster than w_forward there) -- same stored-activation format.
    // GPE_WIDE=1: forward too; GPE_WIDE=0: cooperative kernels only (1D/2D)
    const int wmode = env_int("GPE_WIDE", -1);
    if (uniform && Lh >= 2 && (H == 256 || (H == 128 && dim == 3))) { fused_ok = true; e->wide = true; e->wide_fwd = true; }
    else if (uniform && Lh >= 2 && H == 128 && wmode != 0) { fused_ok = true; e->wide = true; e->wide_fwd = wmode == 1; }
    if (c.path == GPE_PATH_FUSED && !fused_ok)
        CFAIL("fused path needs >=2 hidden layers of one width: 32 or 64 (P*4 <= 160KB LDS), 128 or 256");
    e->path = (c.path == GPE_PATH_GENERIC || !fused_ok) ? GPE_PATH_GENERIC : GPE_PATH_FUSED;
    e->H = H;
    if (e->path == GPE_PATH_FUSED) {
        // f_forward is compiled for GPE_FWD_WAVES resident workgroups per CU (__launch_bounds__): more cannot be honoured by this build
        e->fwd_wg_per_cu = env_int("GPE_FWD_WG_PER_CU", e->fwd_wg_per_cu);
        if (e->fwd_wg_per_cu < 1 || e->fwd_wg_per_cu > GPE_FWD_WAVES)
            CFAIL("GPE_FWD_WG_PER_CU=%d: this build runs f_forward at 1..%d workgroups per CU (more need a build with -DGPE_FWD_WAVES raised to match)",
                  e->fwd_wg_per_cu, GPE_FWD_WAVES);
    }
    return GPE_OK;
}
#undef CFAIL

// the device and the stream: the first HIP call of creation
static int open_device(gpe_engine* e, int device, void* hip_stream) {
    e->device = device; e->stream = (hipStream_t)hip_stream;
    hipError_t st = hipSetDevice(device);
    if (st != hipSuccess) { e->err = std::string("hipSetDevice: ") + hipGetErrorString(st); return GPE_ERR_HIP; }
    if (hipDeviceProp_t prop; hipGetDeviceProperties(&prop, device) == hipSuccess) e->num_cu = prop.multiProcessorCount;
    return GPE_OK;
}

struct AllocSwitches { bool update_multi = true, side_stream = true; };     // switches that only decide what alloc_state allocates

// 5. every remaining GPE_* switch; allocates nothing.  What select_path fixed is not reopened here (see there).
static void read_switches(gpe_engine* e, AllocSwitches& sw) {
    const int H = e->H, Lh = e->nd.n_lin - 1, no = e->nd.n_out;
    // GPE_UPDATE_MULTI=0: the single-workgroup update at every size; GPE_UPDATE_MULTI_MIN (tests): the multi-workgroup form from this many parameters on
    sw.update_multi = e->P >= env_int("GPE_UPDATE_MULTI_MIN", UPD_MULTI_MIN) && env_on("GPE_UPDATE_MULTI");
    e->update_cache = env_on("GPE_UPDATE_CACHE");
    e->fuse_seed = env_on("GPE_FUSE_SEED"); e->fuse_seed_max = env_i64("GPE_FUSE_SEED_MAX", e->fuse_seed_max);
    e->pipe_share = env_int("GPE_PIPE_SHARE", e->pipe_share);
    e->share_min_tiles = env_int_in("GPE_SHARE_MIN_TILES", e->share_min_tiles, 1, INT32_MAX);
    e->fwd_share = env_int("GPE_FWD_SHARE", e->fwd_share);
    e->fuse_head = env_on("GPE_FUSE_HEAD");
    e->fuse_head_tile_min = env_i64("GPE_FUSE_HEAD_TILE_MIN", e->fuse_head_tile_min); e->fuse_head_max = env_i64("GPE_FUSE_HEAD_MAX", e->fuse_head_max);
    // opt-in: measured 1 us SLOWER than the two launches at 2 048 .. 65 536 points (profiles/r04/small_batch.txt) -- 200 workgroups'
    // tickets on one address (~12 ns apiece) and the write-through hand-off cost what the saved launch gives
    e->fuse_update = env_opt_in("GPE_FUSE_UPDATE");
    // opt-in as well: measured EQUAL to the single-workgroup update (35.8 vs 35.7 us at 2 048 points, 41.4 vs 41.0 at 4 000,
    // profiles/r04/small_batch.txt) -- at these sizes a dependent launch costs ~4 us whatever it runs, and the update's own chain is short
    e->split_update = env_opt_in("GPE_SPLIT_UPDATE");
    if (e->path == GPE_PATH_FUSED) {
        e->wide_min_tiles = env_i64_in("GPE_WIDE_MIN_TILES", e->wide_min_tiles, 0, INT64_MAX);
        const int Cmain = e->nd.dim + 2;        // training batches: value, dim first derivatives, Laplacian
        const size_t wb = (size_t)(Lh - 1) * H * H * sizeof(float);
        // (smallb, and the bwd_racc bound that adds it to the kernel's own operands, differ from fused_small_bytes() by a few bytes on purpose)
        const size_t smallb = ((size_t)(4 + (Lh - 1) + no) * H + 8) * sizeof(float);
        e->fwd_wlds = env_on("GPE_WLDS") && H <= 64 && wb + smallb <= 64 * 1024;          // 0 = weights from L2, 1 = from LDS
        e->fwd_b6 = env_opt_in("GPE_FWD_B6") && H <= 64;                 // 1: f_forward_b6 for the large-batch forward pass at H <= 64
        e->bwd_b6 = env_opt_in("GPE_BWD_B6") && H <= 64 && H >= 32;      // 1: the cooperative reverse kernel's adjoint products on the bf16 pipe
        e->bwd_pipe = env_on("GPE_PIPE");                                // 0: the two-barrier cooperative reverse kernel (f_backward_coop) at H <= 64
        e->coop_wg_per_cu = env_int_in("GPE_COOP_WG_PER_CU", e->coop_wg_per_cu, 1, 2);
        e->coop = env_int("GPE_COOP", 1); e->coop_max_tiles = env_i64("GPE_COOP_MAX_TILES", 0);   // (on: measured faster than the per-wave-tile kernels at every batch size)
        e->coop128 = env_on("GPE_COOP128"); e->coop_fwd128 = env_on("GPE_COOP_FWD128");
        e->coop_fwd_max_tiles = env_i64("GPE_COOP_FWD_MAX_TILES", (int64_t)e->num_cu * 8);   // measured: wins below ~32 768 points, loses 8 % at 1M
        e->stage_min_tiles = env_i64("GPE_STAGE_MIN_TILES", 0);          // batches with fewer tiles take the unstaged per-wave-tile kernels
        e->bwd_racc = env_on("GPE_RACC") && H <= 64 && (Lh - 1) >= 1 && (Lh - 1) <= 3 &&
                      ((size_t)e->Ppad + 4 * (size_t)H + 4 * (size_t)Cmain * F_TILE) * sizeof(float) + smallb + wb <= 160 * 1024;
    }
    e->gen_mfma = env_on("GPE_GEN_MFMA"); e->gen_mfma2 = env_on("GPE_GEN_MFMA2");
    e->gen_min_chunk = (env_i64_in("GPE_GEN_MIN_CHUNK", e->gen_min_chunk, 16, INT64_MAX) + 15) / 16 * 16;
    e->head_wg_per_cu = env_int_in("GPE_HEAD_WG_PER_CU", e->head_wg_per_cu, 1, INT32_MAX);
    if (const int ht = env_int("GPE_HEAD_THREADS", e->head_threads); ht == 256 || ht == 512 || ht == 1024) e->head_threads = ht;
    e->merge_bc = env_on("GPE_MERGE_BC");
    // gpe_run replays captured graphs of graph_steps steps each.  Round 4: ONE graph launch per 8 steps takes the host from 31 to
    // 3 us per step at 2 048 points with the step time unchanged (35.5 us: the GPU is the bound); a one-step graph is slower (44.8 us).
    // Default: on for batches up to graph_max_points (where the host thread was ~90 % busy enqueueing); GPE_GRAPH=0 / 1 forces it
    e->use_graph = env_on("GPE_GRAPH"); e->graph_forced = env_set("GPE_GRAPH");
    e->graph_steps = env_int_in("GPE_GRAPH_STEPS", e->graph_steps, 1, 64);
    sw.side_stream = env_on("GPE_SIDE_STREAM");
}

// 6. every device allocation of creation, the side stream and its events
static int alloc_state(gpe_engine* e, const AllocSwitches& sw) {
    const int H = e->H, Lh = e->nd.n_lin - 1;
    e->cap = e->cfg.history_capacity > 0 ? e->cfg.history_capacity : 65536;
    auto alloc = [&](void** p, size_t bytes) -> bool {
        hipError_t s2 = hipMalloc(p, bytes + 256);
        if (s2 != hipSuccess) { e->err = std::string("hipMalloc: ") + hipGetErrorString(s2); return false; }
        (void)hipMemset(*p, 0, bytes + 256);
        return true;
    };
    bool ok = alloc((void**)&e->theta, (size_t)e->P * 4) && alloc((void**)&e->am, (size_t)e->P * 4) &&
              alloc((void**)&e->av, (size_t)e->P * 4) && alloc((void**)&e->grad, ((size_t)e->P + GT_COUNT) * 4) &&
              alloc((void**)&e->dbl, DBL_COUNT * sizeof(double)) && alloc((void**)&e->od, sizeof(OptDev)) &&
              alloc((void**)&e->hist, (size_t)e->cap * sizeof(gpe_scalars)) && alloc((void**)&e->last, sizeof(gpe_scalars)) &&
              alloc((void**)&e->orth_dev, 8 * sizeof(float*));
    if (ok && sw.update_multi) ok = alloc((void**)&e->upd_snap, sizeof(UpdSnap));
    if (ok && e->fuse_head) ok = alloc((void**)&e->head_slots, (size_t)HEAD_SLOTS * 4 * sizeof(double));
    if (ok && e->fuse_update) ok = alloc((void**)&e->upd_ticket, 64);
    if (ok && e->split_update && !e->upd_snap && upd_chunk_host(e->P) <= 1024) ok = alloc((void**)&e->upd_snap_small, sizeof(UpdSnap));
    if (ok && e->path == GPE_PATH_FUSED) {
        e->nslab = (H >= 128) ? std::max(e->nslab_g, e->num_cu) : e->num_cu * 2;     // H = 128: 16 atomic slabs, or one per workgroup (cooperative)
        // WpkT is followed by the bf16 pieces of the same maps (3 x 2 bytes per weight; pack_weight_element, f_forward_b6)
        ok = alloc((void**)&e->Wpk, (size_t)(Lh - 1) * H * H * 4) && alloc((void**)&e->WpkT, (size_t)(Lh - 1) * H * H * (4 + 6 + 6)) &&
             alloc((void**)&e->gslab, (size_t)e->nslab * e->Ppad * 4);
    }
    if (ok) ok = alloc((void**)&e->grad_bc, (size_t)e->P * 4);
    if (ok && e->path == GPE_PATH_FUSED) ok = alloc((void**)&e->gslab_bc, (size_t)e->nslab * e->Ppad * 4);
    if (!ok) return GPE_ERR_NOMEM;
    if (sw.side_stream && (hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking) != hipSuccess ||
                           hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
                           hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess)) {
        e->err = "side stream / events could not be created";
        return GPE_ERR_HIP;
    }
    return GPE_OK;
}

// 7. the kernels that take more dynamic LDS than the 64 KB a launch gets by default: every instance the launchers can pick -- the forms
// and ranges of gpe_dispatch.h, walked with each_* where the launchers pick_* -- once, here (a first launch may sit in a stream capture)
template <class K>
static void lds_limit(K* kernel, int bytes) { (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); }
template <int HH, int CC, int EE, int NO>
static void raise_fused_limits() {
    constexpr int all = 160 * 1024;
    each_int<1, 5>([](auto nh) {
        constexpr int NH = decltype(nh)::value;
        each_int<0, 1>([](auto r) {
            constexpr bool RES = decltype(r)::value;
            if constexpr (coop_form(HH, NO, NH, RES)) lds_limit(f_backward_coop<HH, CC, EE, NO, NH, false, RES>, all);
        });
        if constexpr (HH == 128) lds_limit(f_forward_coop<HH, CC, EE, NO, NH>, all);
        if constexpr (HH <= 64 && NH <= 3) {
            lds_limit(f_backward_coop<HH, CC, EE, NO, NH, true>, all);
            lds_limit(f_backward<HH, CC, EE, NO, true, NH>, all);
            if constexpr (pipe_form(HH, CC)) {
                lds_limit(f_backward_pipe<HH, CC, EE, NO, NH>, all);
                if constexpr (head_form(HH, CC, NO)) lds_limit(f_backward_pipe<HH, CC, EE, NO, NH, true>, all);
            }
        }
    });
    lds_limit(f_backward<HH, CC, EE, NO, false, 0>, all);
    if constexpr (HH <= 64) { lds_limit(f_forward<HH, CC, EE, NO, true>, 64 * 1024); lds_limit(f_forward_b6<HH, CC, EE, NO, true>, 80 * 1024); }
}
static void raise_lds_limits(gpe_engine* e) {
    if (e->path == GPE_PATH_FUSED) {
        if (e->wide) wide_init();
        each_n_out([](auto no) {
            constexpr int NO = decltype(no)::value;
            each_ce(ce_train{}, [](auto CC, auto EE) { raise_fused_limits<64, CC, EE, NO>(); });
#ifndef GPE_FAST_BUILD
            each_ce(ce_train{}, [](auto CC, auto EE) { raise_fused_limits<32, CC, EE, NO>(); });
            each_ce(ce_h128_reverse{}, [](auto CC, auto EE) { raise_fused_limits<128, CC, EE, NO>(); });      // (H = 128: the cooperative forward takes these pairs too, (5,2) goes to f_forward)
#endif
        });
    }
    each_ce(ce_train{}, [](auto CC, auto EE) { lds_limit(g_bwd_weight_mfma2<CC, EE>, 160 * 1024); });
}

extern "C" {

int gpe_abi_version(void) { return GPE_ABI_VERSION; }
size_t gpe_sizeof_config(void) { return sizeof(gpe_config); }
size_t gpe_sizeof_scalars(void) { return sizeof(gpe_scalars); }
size_t gpe_sizeof_observables(void) { return sizeof(struct gpe_observables); }
size_t gpe_sizeof_mixture_observables(void) { return sizeof(struct gpe_mixture_observables); }
size_t gpe_sizeof_sampler_spec(void) { return sizeof(gpe_sampler_spec); }
int64_t gpe_exchange_dbl_count(void) { return DBL_COUNT; }

int gpe_use_external_exchange(gpe_engine* e, void* d_dbl, int64_t n_dbl, void* d_grad, int64_t n_grad) {
    if (!e || !d_dbl || !d_grad) return GPE_ERR_INVALID;
    if (n_dbl < DBL_COUNT || n_grad < e->P + GT_COUNT) FAIL(e, GPE_ERR_INVALID, "external exchange buffers too small");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (!e->ext_exchange) { (void)hipFree(e->dbl); (void)hipFree(e->grad); }
    e->dbl = (double*)d_dbl; e->grad = (float*)d_grad; e->ext_exchange = true;
    e->acc_clean = false;                        // caller-owned buffers: the next step starts with k_begin
    return GPE_OK;
}

const char* gpe_last_error(const gpe_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int gpe_active_path(const gpe_engine* e) { return e ? e->path : GPE_ERR_INVALID; }

// names of the two dominant kernels the bound collocation batch runs (what bench.py prints as roofline.kernel, and what the
// variant tests assert): "fwd=<...>;bwd=<...>"
int gpe_active_kernels(gpe_engine* e, char* buf, size_t n) {
    if (!e || !buf || n == 0) return GPE_ERR_INVALID;
    if (e->main.n <= 0) FAIL(e, GPE_ERR_STATE, "active_kernels before bind_points");
    const Batch& b = e->main;
    char f[160], r[160];
    const int maps = e->nd.n_lin - 2;
    if (e->path == GPE_PATH_FUSED && e->wide) {
        if (e->wide_fwd) snprintf(f, sizeof f, "%s<%d,%d,%d,%d>", wide_forward_kernel(e->H), e->H, b.C, b.E, e->nd.n_out);
        else if (fwd_coop(e, b)) snprintf(f, sizeof f, "f_forward_coop<%d,%d,%d,%d,%d>", e->H, b.C, b.E, e->nd.n_out, maps > 5 ? 5 : maps);
        else snprintf(f, sizeof f, "f_forward<%d,%d,%d,%d,l2>", e->H, b.C, b.E, e->nd.n_out);
        if (wide_reverse(e, const_cast<Batch&>(b))) snprintf(r, sizeof r, "%d x w_bwd_map<%d,%d,%d,%d> (output layer fused into the top map)", maps, e->H, b.C, b.E, e->H / 128);
        else snprintf(r, sizeof r, "f_backward_coop<%d,%d,%d,%d,%d>", e->H, b.C, b.E, e->nd.n_out, maps > 5 ? 5 : maps);
    } else if (e->path == GPE_PATH_FUSED) {
        const bool fc = fwd_coop(e, b);
        if (fc) snprintf(f, sizeof f, "f_forward_coop<%d,%d,%d,%d,%d>", e->H, b.C, b.E, e->nd.n_out, maps > 5 ? 5 : maps);
        else if (e->H <= 64 && e->fwd_b6 && staged_batch(e, b)) snprintf(f, sizeof f, "f_forward_b6<%d,%d,%d,%d>", e->H, b.C, b.E, e->nd.n_out);
        else snprintf(f, sizeof f, "f_forward<%d,%d,%d,%d,%s>", e->H, b.C, b.E, e->nd.n_out,
                      (e->H <= 64 && e->fwd_wlds && staged_batch(e, b)) ? "wlds" : "l2");
        const int kind = bwd_kind(e, b);
        if (kind == 3 && use_pipe(e, b.C)) snprintf(r, sizeof r, "f_backward_pipe<%d,%d,%d,%d,%d%s>", e->H, b.C, b.E, e->nd.n_out, maps,
                                                    seed_in_reverse(e) ? ",seeds" : "");
        else if (kind == 3) snprintf(r, sizeof r, "f_backward_coop<%d,%d,%d,%d,%d%s>", e->H, b.C, b.E, e->nd.n_out, maps > 5 ? 5 : maps,
                                coop_b6(e) ? ",b6" : "");
        else if (kind == 2) snprintf(r, sizeof r, "f_backward<%d,%d,%d,%d,wlds,racc%d>", e->H, b.C, b.E, e->nd.n_out, maps > 3 ? 3 : maps);
        else snprintf(r, sizeof r, "f_backward<%d,%d,%d,%d,l2,%s>", e->H, b.C, b.E, e->nd.n_out, e->H > 64 ? "gacc" : "ldsacc");
        // (whole steps, gpe_step / gpe_run: the split-phase protocol of the data-parallel driver keeps k_head_pde)
        if (fc ? head_fusable_coop(e) : head_fusable_tile(e))
            snprintf(f + strlen(f) - 1, sizeof f - strlen(f) + 1, ",head>");
    } else {
        const int W = e->nd.width[1];
        const bool m2 = e->gen_mfma && e->gen_mfma2 && W % 256 == 0, m1 = e->gen_mfma && W % 64 == 0;
        snprintf(f, sizeof f, "%s<%d,%d>", m2 ? "g_fwd_layer_mfma2" : (m1 ? "g_fwd_layer_mfma" : "g_fwd_layer"), b.C, b.E);
        snprintf(r, sizeof r, "%s<%d,%d>", (e->gen_mfma && e->gen_mfma2 && W % 128 == 0) ? "g_bwd_weight_mfma2"
                                            : (m1 ? "g_bwd_weight_mfma" : "g_bwd_weight"), b.C, b.E);
    }
    // uneven static tile split between the two workgroups of a CU (large batches), where launch_f_forward / launch_f_backward_coop ask for it
    int sf = 0, sb = 0;
    if (e->path == GPE_PATH_FUSED && !e->wide && e->H <= 64) {
        if (!fwd_coop(e, b) && !e->fwd_b6) sf = fwd_tile_share(e, b, fwd_grid(e, b, false));
        if (bwd_kind(e, b) == 3 && use_pipe(e, b.C) && !seed_in_reverse(e)) sb = pipe_tile_share(e, b, fused_grid(e, b.n, 1, e->coop_wg_per_cu));
    }
    if (e->umap.empty()) snprintf(buf, n, "fwd=%s;bwd=%s;split=fwd %d/1024, bwd %d/1024", f, r, sf, sb);
    else snprintf(buf, n, "fwd=%s;bwd=%s;split=fwd %d/1024, bwd %d/1024;padded=hidden widths up to %d run as %d", f, r, sf, sb,
                  *std::max_element(e->user_layers + 1, e->user_layers + e->cfg.n_layers - 1), e->cfg.layers[1]);
    if (e->cfg.mixture) {      // a mixture always takes the standalone pair of its own (the fused head / seeds are real-psi only)
        const size_t used = strlen(buf);
        const char* wqs = e->wq ? ",weighted" : "";
        const char* ens = e->mix_wE != 0.f ? ",energy" : "";
        snprintf(buf + used, n - used, ";head=k_head_mix<%d,%d%s%s>;seed=k_seed_mix<%d,%d%s%s>", b.C, b.E, wqs, ens, b.C, b.E, wqs, ens);
    } else if (e->wq) {      // bound quadrature weights: head and seeds by the standalone kernels' weighted instances, whatever the batch size
        const size_t used = strlen(buf);
        snprintf(buf + used, n - used, ";head=k_head_pde<%d,%d,weighted>;seed=k_seed_pde<%d,%d,weighted>", b.C, b.E, b.C, b.E);
    }
    return GPE_OK;
}

int64_t gpe_param_count(const gpe_engine* e) { return e ? e->P_user : -1; }   /* the caller's network (hidden widths as given) */

int gpe_create(const gpe_config* cfg, int device, void* hip_stream, gpe_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return GPE_ERR_INVALID; }
    *out = nullptr;
    gpe_engine* e = new gpe_engine();
    AllocSwitches sw;
    int rc = check_config(e, *cfg);
    if (!rc) { pad_widths(e); rc = describe_net(e); }
    if (!rc) rc = select_path(e);
    if (!rc) rc = open_device(e, device, hip_stream);
    if (!rc) { read_switches(e, sw); rc = alloc_state(e, sw); }
    if (!rc) { raise_lds_limits(e); fill_phys(e); rc = reset_opt(e, e->cfg.lr); }
    const float pad_b = -40.f;                    // (the padding's biases are in place before the first gpe_set_params, too)
    for (size_t i = 0; !rc && i < e->pad_bias.size(); ++i)
        if (hipMemcpy(e->theta + e->pad_bias[i], &pad_b, sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { e->err = "hipMemcpy (padding)"; rc = GPE_ERR_HIP; }
    if (rc) { g_create_error = e->err; delete e; return rc; }
    *out = e;
    return GPE_OK;
}

static void graph_drop(gpe_engine* e);
int gpe_comm_destroy(gpe_engine* e);

static void orth_state_free(OrthState& s) {      // the stream is idle, or hipFree waits for it
    for (float* p : {s.theta, s.Wpk, s.WpkT, s.psi}) if (p) (void)hipFree(p);
    s = OrthState();
}

static void sampler_free(gpe_engine* e);
static void monitor_free(gpe_engine* e);
void gpe_destroy(gpe_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    if (e->side) { (void)hipStreamSynchronize(e->side); (void)hipStreamDestroy(e->side); }
    (void)gpe_comm_destroy(e);
    graph_drop(e);
    if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    free_batch(e->main); free_batch(e->bc); free_batch(e->sym); free_batch(e->aux); free_batch(e->mse); free_batch(e->orb);
    for (int k = 0; k < GPE_MAX_ORTH; ++k) orth_state_free(e->ost[k]);
    for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
    if (e->ext_exchange) { e->grad = nullptr; e->dbl = nullptr; }
    void* ps[] = {e->theta, e->am, e->av, e->grad, e->dbl, e->od, e->hist, e->last, (void*)e->orth_dev, e->Wpk, e->WpkT, e->gslab, e->gslab_bc, e->grad_bc, (void*)e->upd_snap, (void*)e->head_slots, (void*)e->upd_ticket, (void*)e->upd_snap_small, (void*)e->obs_buf, (void*)e->obs_out, (void*)e->smp.wq_red, (void*)e->pot.V, (void*)e->pot.Vtmp};
    for (void* p : ps) if (p) (void)hipFree(p);
    sampler_free(e);
    monitor_free(e);                              // (the keeper with it)
    lbfgs_free(e);
    delete e;
}

int gpe_synchronize(gpe_engine* e) {
    if (!e) return GPE_ERR_INVALID;
    if (e->side) HIPCHK(e, hipStreamSynchronize(e->side));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

// caller's flat vector (P_user entries, hidden widths as given) <-> the engine's (P entries, padded widths)
static int flat_to_device(gpe_engine* e, float* d_dst, const float* h_user, bool params = false) {
    if (e->umap.empty()) { HIPCHK(e, hipMemcpyAsync(d_dst, h_user, (size_t)e->P * 4, hipMemcpyHostToDevice, e->stream)); return GPE_OK; }
    std::vector<float> tmp((size_t)e->P, 0.f);
    if (params) for (int i : e->pad_bias) tmp[i] = -40.f;         // (parameters only: the Adam moments of the padding are 0)
    for (int i = 0; i < e->P_user; ++i) tmp[e->umap[i]] = h_user[i];
    HIPCHK(e, hipMemcpyAsync(d_dst, tmp.data(), (size_t)e->P * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));              // tmp dies with this frame
    return GPE_OK;
}
static int flat_from_device(gpe_engine* e, const float* d_src, float* h_user) {
    if (e->umap.empty()) { HIPCHK(e, hipMemcpyAsync(h_user, d_src, (size_t)e->P * 4, hipMemcpyDeviceToHost, e->stream)); return GPE_OK; }
    std::vector<float> tmp((size_t)e->P);
    HIPCHK(e, hipMemcpyAsync(tmp.data(), d_src, (size_t)e->P * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int i = 0; i < e->P_user; ++i) h_user[i] = tmp[e->umap[i]];
    return GPE_OK;
}

int gpe_set_params(gpe_engine* e, const float* h, size_t n) {
    if (!e || !h) return GPE_ERR_INVALID;
    if ((int64_t)n != e->P_user) FAIL(e, GPE_ERR_INVALID, "set_params: got %zu floats, model has %d", n, e->P_user);
    int rc = flat_to_device(e, e->theta, h, /*params=*/true);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->packed_dirty = true;
    return lbfgs_reset(e);                        // new parameters: the curvature pairs belong to the old ones
}
int gpe_get_params(gpe_engine* e, float* h, size_t n) {
    if (!e || !h) return GPE_ERR_INVALID;
    if ((int64_t)n != e->P_user) FAIL(e, GPE_ERR_INVALID, "get_params: got %zu floats, model has %d", n, e->P_user);
    int rc = flat_from_device(e, e->theta, h);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}
int gpe_get_grad(gpe_engine* e, float* h, size_t n) {
    if (!e || !h) return GPE_ERR_INVALID;
    if ((int64_t)n != e->P_user) FAIL(e, GPE_ERR_INVALID, "get_grad: size mismatch");
    int rc = flat_from_device(e, e->grad, h);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}
static int opt_state_read(gpe_engine* e, OptDev* h) { return record_copy(e, h, (const OptDev*)e->od, hipMemcpyDeviceToHost); }
static int opt_state_write(gpe_engine* e, const OptDev& h) { return record_copy(e, e->od, &h, hipMemcpyHostToDevice); }
static int last_record_read(gpe_engine* e, gpe_scalars* out) { return record_copy(e, out, (const gpe_scalars*)e->last, hipMemcpyDeviceToHost); }
int gpe_get_adam_state(gpe_engine* e, float* hm, float* hv, size_t n, int64_t* step) {
    if (!e) return GPE_ERR_INVALID;
    if ((int64_t)n != e->P_user) FAIL(e, GPE_ERR_INVALID, "get_adam_state: size mismatch");
    OptDev h;
    int rc;
    if (hm && (rc = flat_from_device(e, e->am, hm))) return rc;
    if (hv && (rc = flat_from_device(e, e->av, hv))) return rc;
    if ((rc = opt_state_read(e, &h))) return rc;
    if (step) *step = h.step;
    return GPE_OK;
}
int gpe_set_adam_state(gpe_engine* e, const float* hm, const float* hv, size_t n, int64_t step) {
    if (!e || !hm || !hv) return GPE_ERR_INVALID;
    if ((int64_t)n != e->P_user) FAIL(e, GPE_ERR_INVALID, "set_adam_state: size mismatch");
    OptDev h;
    if (int rc = opt_state_read(e, &h)) return rc;
    h.step = step;
    h.b1p = pow((double)e->oc.beta1, (double)step); h.b2p = pow((double)e->oc.beta2, (double)step);
    int rc;
    if ((rc = flat_to_device(e, e->am, hm))) return rc;
    if ((rc = flat_to_device(e, e->av, hv))) return rc;
    return opt_state_write(e, h);
}
int gpe_reset_optimizer(gpe_engine* e, float lr) {
    if (!e) return GPE_ERR_INVALID;
    e->cfg.lr = lr;
    return reset_opt(e, lr);
}

static bool precomputed_base(const gpe_engine* e) { return e->cfg.base_mode >= 0 && e->cfg.base_kind == GPE_BASE_PRECOMPUTED; }
// (re)build the collocation batch from what is bound; decides whether the boundary points ride in it
// a precomputed base lives on the bound points: a monitor on them (the only one allowed then) does not outlive a new bind
static void monitor_drop_if_on_bound_points(gpe_engine* e) {
    if (e->mon.bound() && precomputed_base(e)) monitor_free(e);
}

static int rebuild_main(gpe_engine* e) {
    if (!e->ux) return GPE_OK;
    const bool merged = e->merge_bc && e->uxb && e->nb_user > 0 && e->nb_user * 8 <= e->n_pde;
    const int64_t n_tot = e->n_pde + (merged ? e->nb_user : 0);
    int rc = setup_batch(e, e->main, e->ux, n_tot, e->nd.dim + 2, 1, true, e->uV);     // value, dim first derivatives, Laplacian
    if (rc) return rc;
    e->main.pts = Pts{e->ux, merged ? e->uxb : nullptr, e->n_pde};
    e->nb_merged = merged ? e->nb_user : 0;
    if (merged) free_batch(e->bc);
    else if (e->uxb && e->nb_user > 0) { if ((rc = setup_batch(e, e->bc, e->uxb, e->nb_user, 1, 0, false, nullptr))) return rc; }
    else free_batch(e->bc);
    return GPE_OK;
}

// ---- analytic potential terms: the engine-owned V (gpe_potential.h) ----
// V[i] = V(x[i, :]) from the bound table, enqueued on the engine's stream; nothing synchronises.  Never recorded into a graph: the binds,
// sampler_launch and gpe_potential_terms are its callers, and a capture does none of these.
static int pot_fill(gpe_engine* e, const float* x, int64_t n, float* V) {
    hipLaunchKernelGGL(k_potential_terms, dim3(cdiv(n, POT_THREADS)), dim3(POT_THREADS), 0, e->stream, e->pot.tab, e->pot.n, e->nd.dim, x, n, V);
    HIPCHK(e, hipGetLastError());
    return GPE_OK;
}
// room for n values in a buffer that nothing enqueued reads (the stream is idle: callers synchronise first); a buffer of the right
// size stays where it is, so a re-bind of as many rows moves no pointer
static int pot_reserve(gpe_engine* e, const char* who, float** buf, int64_t* have, int64_t n) {
    if (*buf && *have == n) return GPE_OK;
    float* p = nullptr;
    if (hipMalloc((void**)&p, (size_t)n * sizeof(float) + 256) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(e, GPE_ERR_NOMEM, "%s: no memory for the potential on %lld points", who, (long long)n);
    }
    if (*buf) (void)hipFree(*buf);
    *buf = p; *have = n;
    return GPE_OK;
}
// the engine's V takes the place of a caller's d_V on the precomputed-potential path
static bool pot_serves(const gpe_engine* e) { return e->cfg.potential == GPE_POT_PRECOMPUTED && e->pot.on(); }

static void weights_clear(gpe_engine* e) { e->wq = nullptr; e->wq_local = 0.0; e->wq_total = 0.0; }      // (callers run fill_phys)
static int orth_resize(gpe_engine* e);
static int orth_refill(gpe_engine* e);

// the bind itself, shared by gpe_bind_points (caller's points) and gpe_bind_sampler (the engine's own buffer)
static int bind_points_impl(gpe_engine* e, const float* d_x, int64_t n_local, const float* d_V) {
    monitor_drop_if_on_bound_points(e);
    weights_clear(e);                            // weights belong to rows: the new set starts without
    e->ux = d_x; e->uV = d_V; e->n_pde = n_local;
    int rc = rebuild_main(e);
    if (rc) return rc;
    if (e->cfg.w_sym != 0.f) {
        // symmetry batch: [x ; -x], value only
        if (e->sym.n != 2 * n_local) {
            free_batch(e->sym);
            float* xs = nullptr;
            Batch tmp;
            if ((rc = dev_alloc(e, &tmp, &xs, (size_t)2 * n_local * e->nd.dim))) return rc;
            if ((rc = setup_batch(e, e->sym, xs, 2 * n_local, 1, 0, false, nullptr))) return rc;
            e->sym.allocs.push_back(tmp.allocs[0]);
            e->sym.xown = xs;
        }
        hipLaunchKernelGGL(k_make_sym_points, dim3(cdiv(n_local * e->nd.dim, 256)), dim3(256), 0, e->stream, d_x,
                           e->sym.xown, n_local, e->nd.dim);
        HIPCHK(e, hipGetLastError());
    }
    if ((rc = orth_resize(e))) return rc;
    fill_phys(e);
    e->acc_clean = false;
    if (!e->smp.bound() && (rc = orth_refill(e))) return rc;      // (a sampler's set does not exist yet: sampler_launch fills behind its draw)
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

int gpe_bind_points(gpe_engine* e, const float* d_x, int64_t n_local, const float* d_V) {
    if (!e) return GPE_ERR_INVALID;
    if (!d_x || n_local <= 0) FAIL(e, GPE_ERR_INVALID, "bind_points: need n_local > 0 points");
    if (pot_serves(e) && d_V) FAIL(e, GPE_ERR_INVALID, "bind_points: potential terms are bound, and the engine fills V itself (pass d_V = NULL, or clear the terms)");
    if (e->cfg.potential == GPE_POT_PRECOMPUTED && !d_V && !pot_serves(e)) FAIL(e, GPE_ERR_INVALID, "precomputed potential requested but d_V is NULL");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (pot_serves(e)) {                         // V of the new set, filled before anything of the engine changes: a failure leaves it as it was
        if (e->side) HIPCHK(e, hipStreamSynchronize(e->side));
        const bool fresh = !(e->pot.V && e->pot.nV == n_local);      // (a buffer of the right size stays where it is)
        float* nv = e->pot.V;
        if (fresh && hipMalloc((void**)&nv, (size_t)n_local * sizeof(float) + 256) != hipSuccess) {
            (void)hipGetLastError();
            FAIL(e, GPE_ERR_NOMEM, "bind_points: no memory for the potential on %lld points", (long long)n_local);
        }
        if (int rc = pot_fill(e, d_x, n_local, nv)) { if (fresh) (void)hipFree(nv); return rc; }
        if (fresh) {                             // the old buffer goes; uV / main.V, which may still name it, are set by the bind below, and nothing returns in between
            if (e->pot.V) (void)hipFree(e->pot.V);
            e->pot.V = nv; e->pot.nV = n_local;
        }
        d_V = e->pot.V;
    }
    sampler_free(e);                             // the caller's points take over
    return bind_points_impl(e, d_x, n_local, d_V);
}

// ---- device-side stratified sampler ------------------------------------------------------------------------
// what a re-bind replaces but the point buffer: edges, weights, adaptive buffers, the list (the stream is idle); bound weights that were
// the sampler's own go too
static void sampler_free_parts(gpe_engine* e) {
    gpe_engine::Sampler& s = e->smp;
    if (e->wq && e->wq == s.q) weights_clear(e);
    void* ps[] = {s.edges, s.q, s.ad.dev.mass, s.ad.dev.count, s.ad.dev.off, s.ad.dev.share, s.ad.vol, s.ad.resid, s.cl.list};
    for (void* p : ps) if (p) (void)hipFree(p);
    s.edges = nullptr; s.q = nullptr;
    s.edge_off[0] = s.edge_off[1] = s.edge_off[2] = 0;
    s.ad = gpe_engine::Sampler::Adaptive{};
    s.cl = gpe_engine::Sampler::Cells{};
}
// everything: no sampler is bound behind this (the stream is idle: callers synchronise first).  Only the weight total's scratch stays.
static void sampler_free(gpe_engine* e) {
    sampler_free_parts(e);
    if (e->smp.x) (void)hipFree(e->smp.x);
    double* red = e->smp.wq_red;
    e->smp = gpe_engine::Sampler{};
    e->smp.wq_red = red;
}

// draw `draw` into the point buffer (and the [x ; -x] batch) on the engine's stream; nothing synchronises
// (with_weights: a graded sampler's bind, which writes the cell volumes too -- they do not depend on the draw)
static int sampler_launch(gpe_engine* e, int64_t draw, bool with_weights = false) {
    const gpe_engine::Sampler& s = e->smp;
    const dim3 grid(cdiv(s.n, SMP_THREADS)), block(SMP_THREADS);
    if (s.graded()) {
        const float *e0 = s.edges + s.edge_off[0], *e1 = s.edges + s.edge_off[1], *e2 = s.edges + s.edge_off[2];
        float* qw = with_weights ? s.q : nullptr;
        if (s.adaptive()) {                      // counts and offsets from the masses in ad.dev.mass (all zero at the bind), then rows and weights
            hipLaunchKernelGGL(k_adaptive_alloc, dim3(1), dim3(SMP_AD_THREADS), 0, e->stream, s.ad.dev);
            hipLaunchKernelGGL(k_sampler_draw_adaptive, grid, block, 0, e->stream, s.grid, e0, e1, e2, s.ad.dev, (uint64_t)draw, s.x, s.q);
        } else if (s.cells()) {                  // (first + n <= cl.n and every entry < prod shape: checked at the bind)
            hipLaunchKernelGGL(k_sampler_draw_graded_cells, grid, block, 0, e->stream, s.grid, e0, e1, e2, (const int64_t*)s.cl.list, s.first, s.n,
                               (uint64_t)draw, s.x, qw);
        } else {
            hipLaunchKernelGGL(k_sampler_draw_graded, grid, block, 0, e->stream, s.grid, e0, e1, e2, s.first, s.n, (uint64_t)draw, s.x, qw);
        }
    } else {
        float* xs = (e->cfg.w_sym != 0.f && e->sym.n == 2 * s.n) ? e->sym.xown : nullptr;
        if (s.cells())
            hipLaunchKernelGGL(k_sampler_draw_cells, grid, block, 0, e->stream, s.grid, (const int64_t*)s.cl.list, s.first, s.n, (uint64_t)draw, s.x, xs);
        else
            hipLaunchKernelGGL(k_sampler_draw, grid, block, 0, e->stream, s.grid, s.first, s.n, (uint64_t)draw, s.x, xs);
    }
    HIPCHK(e, hipGetLastError());
    e->smp.held = draw;
    // potential terms: V of the new set, behind the draw and before anything reads it -- orth_refill's forward passes do not, the step's
    // head does, and the adaptive detour before the NEXT redraw runs on this set with this V
    if (e->pot_bound()) { int rc = pot_fill(e, s.x, s.n, e->pot.V); if (rc) return rc; }
    return orth_refill(e);                      // frozen orthogonality states: psi_k of the new set, before the step's first kernel
}

// The adaptive sampler's detour, enqueued directly before a redraw: the PDE residual of the current parameters on the set held now, with
// that set's weights, by the launches of gpe_residual up to its seed kernel (k_begin, forward without stored activations, k_head_pde,
// k_seed_pde without seeds), then the block masses.  It writes the step accumulators, the gradient buffers k_begin zeroes and the
// collocation batch's forward buffers -- all of which the step behind it starts by zeroing (acc_clean is false: sampler_before_step;
// a captured graph always starts with k_begin) or overwriting -- and never the parameters, the optimiser state, the scheduler,
// history, `last` or the stop flag: k_update is not launched.  Nothing synchronises or allocates.
static int launch_head_pde(gpe_engine* e, bool energy = false);
static int launch_seed_pde(gpe_engine* e, float* d_resid, int want_seeds, int head_slots);
static int adaptive_masses(gpe_engine* e) {
    const gpe_engine::Sampler& s = e->smp;
    int rc;
    if ((rc = launch_begin(e, /*force=*/true))) return rc;
    if ((rc = mlp_forward(e, e->main, false))) return rc;
    if ((rc = launch_head_pde(e))) return rc;
    if ((rc = launch_seed_pde(e, s.ad.resid, 0, /*head_slots=*/0))) return rc;
    const unsigned g = (unsigned)std::min<int64_t>(cdiv((int64_t)s.ad.dev.B, 4), (int64_t)e->num_cu * 4);
    hipLaunchKernelGGL(k_block_mass, dim3(g), dim3(SMP_MASS_THREADS), 0, e->stream, (const float*)s.ad.resid, (const float*)s.q,
                       (const int32_t*)s.ad.dev.off, e->nd.n_out, (int)s.ad.dev.B, s.ad.dev.mass);
    HIPCHK(e, hipGetLastError());
    return GPE_OK;
}

// before the first kernel of a step: the set this step runs on.  A redraw leaves the engine as gpe_bind_points of the new set would
// (the step starts with k_begin; Phys and the merged-boundary Pts depend on the point count and the pointers only, which stay) --
// without that call's two synchronisations.
static int sampler_before_step(gpe_engine* e, bool capturing) {
    const gpe_engine::Sampler& s = e->smp;
    if (!s.bound() || capturing) return GPE_OK;
    const int64_t want = s.draw0 + s.steps / s.every;
    if (want == s.held) return GPE_OK;
    e->acc_clean = false;
    int rc;
    if (s.adaptive() && (rc = adaptive_masses(e))) return rc;
    return sampler_launch(e, want);
}

// one fixed-order fp64 total of a weight array on the engine's stream, read back here: the bind's one synchronisation
static int weights_total(gpe_engine* e, const float* d_q, int64_t n, double* total, double* bad) {
    if (!e->smp.wq_red && hipMalloc((void**)&e->smp.wq_red, 2 * sizeof(double) + 256) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(e, GPE_ERR_NOMEM, "bind_weights: no memory for the weight total");
    }
    hipLaunchKernelGGL(k_weight_total, dim3(1), dim3(WQ_THREADS), 0, e->stream, d_q, n, e->smp.wq_red);
    HIPCHK(e, hipGetLastError());
    double h[2] = {0.0, 0.0};
    HIPCHK(e, hipMemcpyAsync(h, e->smp.wq_red, sizeof h, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    *total = h[0]; *bad = h[1];
    return GPE_OK;
}

// ---- the bind, in phases (sampler_bind calls each once, in this order) ----
// edges NULL: the uniform grid of gpe_bind_sampler, else one host array per used axis; ad (with edges): gpe_sampler_adaptive;
// cl (with or without edges): gpe_sampler_cells -- first_cell / n_local index the list.  who: sampler_who, the name in every message.

// 1. what the engine's own state rules out; nothing is touched
static int sampler_refuse_state(gpe_engine* e, const char* who, bool adaptive) {
    if (adaptive && e->dp.on()) FAIL(e, GPE_ERR_STATE, "%s: the engine has a communicator, and a data-parallel allocation needs a mass exchange", who);
    if (e->cfg.potential == GPE_POT_PRECOMPUTED && !e->pot.on())        // (with terms bound the engine refills its own V behind every draw)
        FAIL(e, GPE_ERR_INVALID, "%s: a precomputed potential lives on fixed points", who);
    if (precomputed_base(e)) FAIL(e, GPE_ERR_INVALID, "%s: a precomputed base lives on fixed points", who);
    for (int k = 0; k < GPE_MAX_ORTH; ++k)       // (a frozen state is re-evaluated behind every redraw: only caller arrays are refused)
        if (e->orth_host[k] && !e->ost[k].on) FAIL(e, GPE_ERR_INVALID, "%s: orthogonality array %d is bound, and lives on fixed points", who, k);
    return GPE_OK;
}

// 2. the plan: gpe_sampler_plan.h (it judges w_sym with edges too, where that refusal has always stood: behind `every`)

// 3a. synchronise; the engine's copy of the list, and a point buffer if the row count changes (*x stays NULL otherwise: the buffer and a
// captured graph's pointers stay).  Nothing of the engine changes: a failure here leaves it as it was.
static int sampler_reserve(gpe_engine* e, const char* who, const CellsArgs* cl, int64_t n_rows, int64_t** d_cells, float** x) {
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->side) HIPCHK(e, hipStreamSynchronize(e->side));
    if (cl) {
        if (hipMalloc((void**)d_cells, (size_t)cl->n_cells * sizeof(int64_t) + 256) != hipSuccess) {
            (void)hipGetLastError();
            FAIL(e, GPE_ERR_NOMEM, "%s: no memory for the list of %lld cells", who, (long long)cl->n_cells);
        }
        if (hipMemcpy(*d_cells, cl->h_cells, (size_t)cl->n_cells * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(*d_cells);
            FAIL(e, GPE_ERR_HIP, "%s: upload of the cell list failed", who);
        }
    }
    if ((e->smp.n != n_rows || !e->smp.x) && hipMalloc((void**)x, (size_t)n_rows * e->nd.dim * sizeof(float) + 256) != hipSuccess) {
        (void)hipGetLastError();
        if (*d_cells) (void)hipFree(*d_cells);
        FAIL(e, GPE_ERR_NOMEM, "%s: no memory for %lld points", who, (long long)n_rows);
    }
    return GPE_OK;
}

// 3b. the old sampler goes -- all of it if a new point buffer x was reserved, else all but the buffer -- and the list, edges, weights and
// adaptive buffers enter the record.  From here on a failure is sampler_bind_failed's.
static int sampler_acquire(gpe_engine* e, const char* who, const gpe_sampler_spec* sp, const float* const* edges, const CellsArgs* cl,
                           const SamplerPlan& plan, int64_t* d_cells, float* x) {
    gpe_engine::Sampler& s = e->smp;
    if (x) { sampler_free(e); s.x = x; }
    else sampler_free_parts(e);
    if (e->mse_target) { e->mse_target = nullptr; free_batch(e->mse); }      // a pre-training target lived on the points that just went
    s.cl.list = d_cells; s.cl.n = cl ? cl->n_cells : 0;
    if (pot_serves(e)) {                         // potential terms: V of the set, beside the point buffer (kept where the row count stays; a failure from here on is
                                                 // sampler_bind_failed's, which leaves nothing bound: uV never outlives a buffer this frees)
        int rc = pot_reserve(e, who, &e->pot.V, &e->pot.nV, plan.n_rows);
        if (rc) return rc;
    }
    if (edges) {
        if (hipMalloc((void**)&s.edges, (size_t)plan.n_edges * sizeof(float) + 256) != hipSuccess ||
            hipMalloc((void**)&s.q, (size_t)plan.n_rows * sizeof(float) + 256) != hipSuccess) {
            (void)hipGetLastError();
            e->err = std::string(who) + ": no memory for the edges and weights";
            return GPE_ERR_NOMEM;
        }
        int64_t off = 0;
        for (int k = 0; k < e->nd.dim; ++k) {    // (unused axes keep offset 0, axis 0: never read)
            s.edge_off[k] = off;
            if (hipMemcpy(s.edges + off, edges[k], (size_t)(sp->shape[k] + 1) * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipGetLastError();
                e->err = std::string(who) + ": upload of the edges failed";
                return GPE_ERR_HIP;
            }
            off += sp->shape[k] + 1;
        }
    }
    if (!plan.vol.empty()) {                     // adaptive: masses (all zero: the bind allocates by volume), counts, offsets, volumes, residual
        const size_t B = plan.vol.size();
        AdaptiveDev& a = s.ad.dev;
        if (hipMalloc((void**)&a.mass, (B + 1) * sizeof(double) + 256) != hipSuccess ||
            hipMalloc((void**)&a.count, B * sizeof(int32_t) + 256) != hipSuccess ||
            hipMalloc((void**)&a.off, (B + 1) * sizeof(int32_t) + 256) != hipSuccess ||
            hipMalloc((void**)&a.share, B * sizeof(uint64_t) + 256) != hipSuccess ||
            hipMalloc((void**)&s.ad.vol, B * sizeof(float) + 256) != hipSuccess ||
            hipMalloc((void**)&s.ad.resid, (size_t)plan.n_rows * e->nd.n_out * sizeof(float) + 256) != hipSuccess) {
            (void)hipGetLastError();
            e->err = std::string(who) + ": no memory for the block masses, counts and the residual";
            return GPE_ERR_NOMEM;
        }
        if (hipMemset(a.mass, 0, (B + 1) * sizeof(double)) != hipSuccess ||
            hipMemcpy(s.ad.vol, plan.vol.data(), B * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            e->err = std::string(who) + ": upload of the block volumes failed";
            return GPE_ERR_HIP;
        }
    }
    return GPE_OK;
}

// 4. the record's scalars, the bind of the buffer as the collocation batch, the first draw and -- graded -- the weights
static int sampler_commit(gpe_engine* e, const char* who, const gpe_sampler_spec* sp, const AdaptiveArgs* ad, const SamplerPlan& plan) {
    gpe_engine::Sampler& s = e->smp;
    SamplerGrid& g = s.grid;
    memset(&g, 0, sizeof g);
    g.dim = e->nd.dim; g.key0 = (uint32_t)sp->seed; g.key1 = (uint32_t)(sp->seed >> 32);
    for (int k = 0; k < g.dim; ++k) {
        g.shape[k] = sp->shape[k]; g.lo[k] = sp->lo[k]; g.clip_lo[k] = sp->clip_lo[k]; g.clip_hi[k] = sp->clip_hi[k];
        g.h[k] = (float)(((double)sp->hi[k] - (double)sp->lo[k]) / (double)sp->shape[k]);
    }
    if (ad) {
        AdaptiveDev& a = s.ad.dev;
        a.vol = s.ad.vol; a.B = (int32_t)sp->n_local; a.N = (int32_t)plan.n_rows; a.n_min = ad->n_min; a.s = ad->s; a.V = plan.w_grid;
    }
    s.n = plan.n_rows; s.first = sp->first_cell; s.every = sp->every; s.draw0 = sp->draw0; s.steps = 0;
    s.held = sp->draw0;
    int rc = bind_points_impl(e, s.x, s.n, pot_serves(e) ? e->pot.V : nullptr);      // (V: filled by the launch below, behind the draw); allocates the symmetry batch; its copy kernel reads a buffer ...
    if (!rc) rc = sampler_launch(e, sp->draw0, /*with_weights=*/s.graded());      // ... this launch fills, together with [x ; -x]
    if (!rc && s.graded()) {                     // the cell volumes become the bound weights, W the whole grid's (or list's) volume
        double wl = 0.0, bad = 0.0;
        rc = weights_total(e, s.q, s.n, &wl, &bad);
        if (!rc && (bad != 0.0 || !(wl > 0.0) || !__builtin_isfinite(wl) || !(plan.w_grid > 0.0) || !__builtin_isfinite(plan.w_grid))) {
            e->err = std::string(who) + ": the cell volumes of this block underflow or overflow fp32"; rc = GPE_ERR_INVALID;
        }
        if (!rc) { e->wq = s.q; e->wq_local = wl; e->wq_total = plan.w_grid; fill_phys(e); }
    }
    if (!rc && hipStreamSynchronize(e->stream) != hipSuccess) { e->err = std::string(who) + ": synchronise failed"; rc = GPE_ERR_HIP; }
    return rc;
}

// 5. never leave a half-bound sampler behind: no sampler, no points, the error text kept
static int sampler_bind_failed(gpe_engine* e, int rc) {
    const std::string keep = e->err;
    (void)hipStreamSynchronize(e->stream);
    sampler_free(e);
    e->ux = nullptr; e->uV = nullptr; e->n_pde = 0; free_batch(e->main); free_batch(e->sym);
    fill_phys(e);
    e->err = keep;
    return rc;
}

static int sampler_bind(gpe_engine* e, const gpe_sampler_spec* sp, const float* const* edges, const AdaptiveArgs* ad = nullptr,
                        const CellsArgs* cl = nullptr) {
    const char* who = sampler_who(edges, ad, cl);
    int rc;
    if ((rc = sampler_refuse_state(e, who, ad != nullptr))) return rc;
    SamplerPlan plan;
    std::string msg;
    if ((rc = sampler_plan(e->nd.dim, e->cfg.w_sym != 0.f, sp, edges, ad, cl, SMP_AD_MAX_POINTS, &plan, &msg))) { e->err = msg; return rc; }
    int64_t* d_cells = nullptr;
    float* x = nullptr;
    if ((rc = sampler_reserve(e, who, cl, plan.n_rows, &d_cells, &x))) return rc;
    if ((rc = sampler_acquire(e, who, sp, edges, cl, plan, d_cells, x))) return sampler_bind_failed(e, rc);
    if ((rc = sampler_commit(e, who, sp, ad, plan))) return sampler_bind_failed(e, rc);
    return GPE_OK;
}

// no points stay bound (the streams are idle): what clearing a sampler leaves, and clearing potential terms whose V the bound set ran on
static int unbind_points(gpe_engine* e) {
    monitor_drop_if_on_bound_points(e);
    graph_drop(e);
    sampler_free(e);                             // (a graded sampler's weights go with it)
    e->ux = nullptr; e->uV = nullptr; e->n_pde = 0;
    free_batch(e->main); free_batch(e->sym);
    if (e->uxb && e->nb_user > 0) { int rc = setup_batch(e, e->bc, e->uxb, e->nb_user, 1, 0, false, nullptr); if (rc) return rc; }
    e->nb_merged = 0;
    e->acc_clean = false;
    fill_phys(e);
    return GPE_OK;
}

int gpe_bind_sampler(gpe_engine* e, const gpe_sampler_spec* sp) {
    if (!e) return GPE_ERR_INVALID;
    if (!sp) {                                   // clear: the buffer goes, so nothing stays bound
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (e->side) HIPCHK(e, hipStreamSynchronize(e->side));
        if (!e->smp.bound()) return GPE_OK;
        return unbind_points(e);
    }
    return sampler_bind(e, sp, nullptr);
}

int gpe_bind_sampler_graded(gpe_engine* e, const gpe_sampler_spec* sp, const float* h_edges0, const float* h_edges1, const float* h_edges2) {
    if (!e) return GPE_ERR_INVALID;
    if (!sp) FAIL(e, GPE_ERR_INVALID, "bind_sampler_graded: no spec (gpe_bind_sampler(NULL) clears a sampler of either kind)");
    const float* edges[3] = {h_edges0, h_edges1, h_edges2};
    return sampler_bind(e, sp, edges);
}

int gpe_sampler_adaptive(gpe_engine* e, const gpe_sampler_spec* sp, const float* h_edges0, const float* h_edges1, const float* h_edges2,
                         int64_t n_points, int32_t n_min, int32_t uniform_per_1024) {
    if (!e) return GPE_ERR_INVALID;
    if (!sp) FAIL(e, GPE_ERR_INVALID, "sampler_adaptive: no spec (gpe_bind_sampler(NULL) clears a sampler of any kind)");
    const float* edges[3] = {h_edges0, h_edges1, h_edges2};
    const AdaptiveArgs ad{n_points, n_min, uniform_per_1024};
    return sampler_bind(e, sp, edges, &ad);
}

int gpe_sampler_cells(gpe_engine* e, const gpe_sampler_spec* sp, const int64_t* h_cells, int64_t n_cells,
                      const float* h_edges0, const float* h_edges1, const float* h_edges2) {
    if (!e) return GPE_ERR_INVALID;
    if (!sp) FAIL(e, GPE_ERR_INVALID, "sampler_cells: no spec (gpe_bind_sampler(NULL) clears a sampler of any kind)");
    if (!h_cells || n_cells <= 0) FAIL(e, GPE_ERR_INVALID, "sampler_cells: need a list of n_cells > 0 cells (n_cells = %lld)", (long long)n_cells);
    const float* edges[3] = {h_edges0, h_edges1, h_edges2};
    bool graded = false;                         // edges on any used axis: graded, and the plan wants them on every used axis
    for (int k = 0; k < e->nd.dim && k < 3; ++k) graded = graded || edges[k] != nullptr;
    const CellsArgs cl{h_cells, n_cells};
    return sampler_bind(e, sp, graded ? edges : nullptr, nullptr, &cl);
}

int gpe_sampler_cells_read(gpe_engine* e, const int64_t** d_cells, int64_t* n_cells, int64_t* first) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->smp.bound() || !e->smp.cells()) FAIL(e, GPE_ERR_STATE, "sampler_cells_read: no cell-subset sampler bound");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (d_cells) *d_cells = e->smp.cl.list;
    if (n_cells) *n_cells = e->smp.cl.n;
    if (first) *first = e->smp.first;
    return GPE_OK;
}

int gpe_sampler_adaptive_blocks(gpe_engine* e, int64_t* n_blocks, int64_t* n_points) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->smp.adaptive()) FAIL(e, GPE_ERR_STATE, "sampler_adaptive_blocks: no adaptive sampler bound");
    if (n_blocks) *n_blocks = e->smp.ad.dev.B;
    if (n_points) *n_points = e->smp.ad.dev.N;
    return GPE_OK;
}

int gpe_sampler_adaptive_state(gpe_engine* e, double* h_mass, double* mass_total, int32_t* h_count, int64_t* draw) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->smp.adaptive()) FAIL(e, GPE_ERR_STATE, "sampler_adaptive_state: no adaptive sampler bound");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const size_t B = (size_t)e->smp.ad.dev.B;
    if (h_mass) HIPCHK(e, hipMemcpy(h_mass, e->smp.ad.dev.mass, B * sizeof(double), hipMemcpyDeviceToHost));
    if (mass_total) HIPCHK(e, hipMemcpy(mass_total, e->smp.ad.dev.mass + B, sizeof(double), hipMemcpyDeviceToHost));
    if (h_count) HIPCHK(e, hipMemcpy(h_count, e->smp.ad.dev.count, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (draw) *draw = e->smp.held;
    return GPE_OK;
}

int gpe_bind_weights(gpe_engine* e, const float* d_q, double w_total) {
    if (!e) return GPE_ERR_INVALID;
    if (!d_q) {                                  // clear: the count-based N is back
        if (e->smp.graded()) FAIL(e, GPE_ERR_STATE, "bind_weights: the graded sampler owns the bound weights (gpe_bind_sampler(NULL) clears both)");
        HIPCHK(e, hipStreamSynchronize(e->stream));
        weights_clear(e);
        fill_phys(e);
        return GPE_OK;
    }
    if (!e->ux || e->n_pde <= 0) FAIL(e, GPE_ERR_STATE, "bind_weights before bind_points");
    if (e->smp.bound()) FAIL(e, GPE_ERR_STATE, "bind_weights: a sampler is bound, its rows move at the next redraw");
    if (e->cfg.w_sym != 0.f) FAIL(e, GPE_ERR_INVALID, "bind_weights: the symmetry batch has no quadrature weights (w_sym != 0)");
    if (!(w_total >= 0.0) || !__builtin_isfinite(w_total)) FAIL(e, GPE_ERR_INVALID, "bind_weights: w_total = %g, need a finite value >= 0 (0: this rank's total)", w_total);
    double wl = 0.0, bad = 0.0;
    int rc = weights_total(e, d_q, e->n_pde, &wl, &bad);
    if (rc) return rc;
    if (bad != 0.0) FAIL(e, GPE_ERR_INVALID, "bind_weights: %.0f of the %lld weights are negative or not finite", bad, (long long)e->n_pde);
    if (!(wl > 0.0) || !__builtin_isfinite(wl)) FAIL(e, GPE_ERR_INVALID, "bind_weights: the weights add up to %g, need a finite total > 0", wl);
    e->wq = d_q; e->wq_local = wl; e->wq_total = w_total > 0.0 ? w_total : wl;
    fill_phys(e);
    return GPE_OK;
}

int gpe_weights(gpe_engine* e, const float** d_q, int64_t* n, double* w_local, double* w_total) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->wq) FAIL(e, GPE_ERR_STATE, "weights: no weights bound");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (d_q) *d_q = e->wq;
    if (n) *n = e->n_pde;
    if (w_local) *w_local = e->wq_local;
    if (w_total) *w_total = e->wq_total;
    return GPE_OK;
}

int gpe_sampler_points(gpe_engine* e, const float** d_x, int64_t* n, int64_t* draw) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->smp.bound()) FAIL(e, GPE_ERR_STATE, "sampler_points: no sampler bound");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (d_x) *d_x = e->smp.x;
    if (n) *n = e->smp.n;
    if (draw) *draw = e->smp.held;
    return GPE_OK;
}

int gpe_bind_boundary(gpe_engine* e, const float* d_xb, int64_t n_b, const float* d_target) {
    if (!e) return GPE_ERR_INVALID;
    if (!d_xb || n_b <= 0) { e->uxb = nullptr; e->nb_user = 0; e->bc_target = nullptr; }
    else { e->uxb = d_xb; e->nb_user = n_b; e->bc_target = d_target; }
    if (e->ux) {
        int rc = rebuild_main(e);
        if (rc) return rc;
    } else if (e->uxb) {             // points not bound yet: keep a plain boundary batch until they are
        int rc = setup_batch(e, e->bc, e->uxb, e->nb_user, 1, 0, false, nullptr);
        if (rc) return rc;
    } else free_batch(e->bc);
    e->acc_clean = false;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

// ---- orthogonality slots: a caller's array on the bound points, or a frozen state the engine evaluates itself ---------------------
static int orth_publish(gpe_engine* e) {         // orth_host -> the device copy the head / seed kernels read; n_orth
    HIPCHK(e, hipMemcpyAsync((void*)e->orth_dev, e->orth_host, sizeof e->orth_host, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    fill_phys(e);
    return GPE_OK;
}

int gpe_bind_orth(gpe_engine* e, int k, const float* d_psi) {
    if (!e || k < 0 || k >= GPE_MAX_ORTH) return GPE_ERR_INVALID;
    if (e->cfg.mixture) FAIL(e, GPE_ERR_STATE, "bind_orth: a mixture engine has no orthogonality term");
    if (d_psi && e->smp.bound()) FAIL(e, GPE_ERR_STATE, "bind_orth: a sampler is bound, an orthogonality array would go stale at its next redraw");
    if (e->ost[k].on) {                          // the array (or NULL) replaces a frozen state
        HIPCHK(e, hipStreamSynchronize(e->stream));
        orth_state_free(e->ost[k]);
    }
    e->orth_host[k] = d_psi;
    return orth_publish(e);
}

// the value-only forward batch of the refills and every frozen state's psi buffer, sized for the bound collocation set; a buffer is
// reallocated only when the point count changed.  The stream is idle (the binds synchronise first).
static int orth_resize(gpe_engine* e) {
    bool any = false;
    for (int k = 0; k < GPE_MAX_ORTH; ++k) any = any || e->ost[k].on;
    if (!any) { if (e->orb.O) free_batch(e->orb); return GPE_OK; }
    if (!e->ux || e->n_pde <= 0) return GPE_OK;
    int rc = setup_batch(e, e->orb, e->ux, e->n_pde, 1, 0, false, nullptr, /*with_store=*/false);
    if (rc) return rc;
    bool moved = false;
    for (int k = 0; k < GPE_MAX_ORTH; ++k) {
        OrthState& s = e->ost[k];
        if (!s.on || s.n == e->n_pde) continue;
        float* p = nullptr;
        if (hipMalloc((void**)&p, (size_t)e->n_pde * sizeof(float) + 256) != hipSuccess) {
            (void)hipGetLastError();
            orth_state_free(s);                   // never leave a buffer of the old size in a slot the head kernels read
            e->orth_host[k] = nullptr;
            (void)orth_publish(e);
            FAIL(e, GPE_ERR_NOMEM, "orthogonality state %d: no memory for %lld values (the slot was cleared)", k, (long long)e->n_pde);
        }
        (void)hipFree(s.psi);
        s.psi = p; s.n = e->n_pde;
        e->orth_host[k] = p;
        moved = true;
    }
    return moved ? orth_publish(e) : GPE_OK;
}

// psi_k of every frozen state on the collocation set bound now: the value-only forward pass on the frozen parameters (the kernel set
// gpe_forward runs), then k_orth_fill.  Enqueued on the engine's stream; nothing synchronises; never recorded into a graph (the binds
// and sampler_launch are its only callers, and a capture neither binds nor redraws).
static int orth_refill(gpe_engine* e) {
    if (!e->ux || e->n_pde <= 0) return GPE_OK;
    for (int k = 0; k < GPE_MAX_ORTH; ++k) {
        const OrthState& s = e->ost[k];
        if (!s.on) continue;
        if (s.n != e->n_pde || e->orb.n != e->n_pde) FAIL(e, GPE_ERR_STATE, "orthogonality state %d: buffers not sized for the bound set", k);
        e->orb.pts = Pts{e->ux, nullptr, e->n_pde};
        const FwdWeights w{s.theta, s.Wpk, s.WpkT};
        int rc = mlp_forward(e, e->orb, false, &w);
        if (rc) return rc;
        Phys ph = e->ph;
        ph.base_mode = s.base_mode; ph.perturb_scale = s.perturb_scale;
        hipLaunchKernelGGL(k_orth_fill, dim3(cdiv(e->n_pde, 256)), dim3(256), 0, e->stream, ph, s.base_norm, e->ux, (const float*)e->orb.O,
                           s.amplitude, s.psi, e->n_pde);
        HIPCHK(e, hipGetLastError());
    }
    return GPE_OK;
}

int gpe_bind_orth_state(gpe_engine* e, int k, const float* h_flat, size_t n, int base_mode, float perturb_scale, float amplitude) {
    if (!e) return GPE_ERR_INVALID;
    if (e->cfg.mixture) FAIL(e, GPE_ERR_STATE, "bind_orth_state: a mixture engine has no orthogonality term");
    if (k < 0 || k >= GPE_MAX_ORTH) FAIL(e, GPE_ERR_INVALID, "bind_orth_state: slot %d, need 0..%d", k, GPE_MAX_ORTH - 1);
    if (!h_flat) return gpe_bind_orth(e, k, nullptr);
    if (e->cfg.complex_psi || e->nd.n_out != 1) FAIL(e, GPE_ERR_INVALID, "bind_orth_state: frozen states need real psi (out=1)");
    if ((int64_t)n != e->P_user) FAIL(e, GPE_ERR_INVALID, "bind_orth_state: got %zu floats, model has %d", n, e->P_user);
    if (base_mode >= 0 && (e->cfg.base_kind == GPE_BASE_PRECOMPUTED || e->nd.dim > 1))
        FAIL(e, GPE_ERR_INVALID, "bind_orth_state: a base needs dim=1 and an analytic base kind (a precomputed base lives on fixed points)");
    if (!isfinite(perturb_scale) || !isfinite(amplitude)) FAIL(e, GPE_ERR_INVALID, "bind_orth_state: perturb_scale / amplitude not finite");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->side) HIPCHK(e, hipStreamSynchronize(e->side));
    // build the new state aside; the slot changes only once everything is in place
    OrthState s;
    const bool have_pts = e->ux && e->n_pde > 0;
    const size_t wn = e->path == GPE_PATH_FUSED ? (size_t)(e->nd.n_lin - 2) * e->H * e->H : 0;
    bool ok = hipMalloc((void**)&s.theta, (size_t)e->P * 4 + 256) == hipSuccess &&
              hipMalloc((void**)&s.psi, (size_t)(have_pts ? e->n_pde : 0) * sizeof(float) + 256) == hipSuccess;
    if (ok && wn) ok = hipMalloc((void**)&s.Wpk, wn * 4 + 256) == hipSuccess && hipMalloc((void**)&s.WpkT, wn * (4 + 6 + 6) + 256) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); orth_state_free(s); FAIL(e, GPE_ERR_NOMEM, "bind_orth_state: no memory for the frozen state"); }
    int rc = flat_to_device(e, s.theta, h_flat, /*params=*/true);
    if (!rc && hipStreamSynchronize(e->stream) != hipSuccess) { e->err = "bind_orth_state: upload failed"; rc = GPE_ERR_HIP; }
    if (!rc && wn) {                             // the same packing as the trained parameters (k_pack_weights / k_begin)
        hipLaunchKernelGGL(k_pack_weights, dim3(cdiv((int64_t)wn, 256)), dim3(256), 0, e->stream, e->nd, e->H, (const float*)s.theta, s.Wpk, s.WpkT);
        if (hipGetLastError() != hipSuccess) { e->err = "bind_orth_state: k_pack_weights launch failed"; rc = GPE_ERR_HIP; }
    }
    if (!rc && have_pts) rc = setup_batch(e, e->orb, e->ux, e->n_pde, 1, 0, false, nullptr, /*with_store=*/false);
    if (rc) { (void)hipStreamSynchronize(e->stream); orth_state_free(s); return rc; }
    s.on = true; s.n = have_pts ? e->n_pde : 0;
    s.base_mode = base_mode; s.perturb_scale = perturb_scale; s.amplitude = amplitude;
    if (base_mode >= 0) {                        // Hermite normalisation, as fill_phys forms the engine's
        double f = 1.0;
        for (int i = 2; i <= base_mode; ++i) f *= i;
        s.base_norm = (float)pow(pow(2.0, base_mode) * f * sqrt(M_PI), -0.5);
    }
    orth_state_free(e->ost[k]);                  // (a caller array in the slot is simply replaced)
    e->ost[k] = s;
    e->orth_host[k] = s.psi;
    if ((rc = orth_publish(e))) return rc;
    if ((rc = orth_refill(e))) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

int gpe_orth_values(gpe_engine* e, int k, const float** d_psi, int64_t* n) {
    if (!e) return GPE_ERR_INVALID;
    if (k < 0 || k >= GPE_MAX_ORTH) FAIL(e, GPE_ERR_INVALID, "orth_values: slot %d, need 0..%d", k, GPE_MAX_ORTH - 1);
    if (!e->ost[k].on) FAIL(e, GPE_ERR_STATE, "orth_values: slot %d holds no frozen state", k);
    if (!e->ux || e->n_pde <= 0 || e->ost[k].n != e->n_pde) FAIL(e, GPE_ERR_STATE, "orth_values: no points bound");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (d_psi) *d_psi = e->ost[k].psi;
    if (n) *n = e->n_pde;
    return GPE_OK;
}

int gpe_bind_base(gpe_engine* e, const float* d_phi, const float* d_phi1, const float* d_phi2) {
    if (!e) return GPE_ERR_INVALID;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    monitor_drop_if_on_bound_points(e);
    e->orth_host[4] = d_phi; e->orth_host[5] = d_phi1; e->orth_host[6] = d_phi2;
    HIPCHK(e, hipMemcpyAsync((void*)e->orth_dev, e->orth_host, sizeof e->orth_host, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

// ---- forward-only ----------------------------------------------------------------------------------
static int aux_forward(gpe_engine* e, const float* d_x, int64_t n, int C, int E) {
    int rc = setup_batch(e, e->aux, d_x, n, C, E, true, nullptr, /*with_store=*/false);
    if (rc) return rc;
    return mlp_forward(e, e->aux, false);
}

int gpe_forward(gpe_engine* e, const float* d_x, int64_t n, float* d_out) {
    if (!e || !d_x || !d_out || n <= 0) return GPE_ERR_INVALID;
    int rc = aux_forward(e, d_x, n, 1, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(k_copy_values, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, e->ph, d_x, e->aux.O, d_out, n, e->aux.ld, e->nd.n_out);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

int gpe_forward_jets(gpe_engine* e, const float* d_x, int64_t n, float* d_jets) {
    if (!e || !d_x || !d_jets || n <= 0) return GPE_ERR_INVALID;
    const int C = 1 + 2 * e->nd.dim;
    int rc = aux_forward(e, d_x, n, C, e->nd.dim);        // full diagonal second derivatives: E = dim
    if (rc) return rc;
    hipLaunchKernelGGL(k_copy_jets, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, e->aux.O, d_jets, n, e->aux.ld, e->nd.n_out, C);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

int gpe_eval_density(gpe_engine* e, const float* d_x, int64_t n, float dx, int abs_flag, float* d_u, float* d_dens) {
    if (!e || !d_x || n <= 0) return GPE_ERR_INVALID;
    if (e->cfg.mixture) FAIL(e, GPE_ERR_STATE, "eval_density: a mixture engine has one norm per component (use gpe_forward and gpe_mixture_scalars)");
    if (e->cfg.base_mode >= 0 && e->cfg.base_kind == GPE_BASE_PRECOMPUTED)
        FAIL(e, GPE_ERR_INVALID, "eval_density needs an analytic base (the precomputed base exists on the bound points only)");
    int rc = aux_forward(e, d_x, n, 1, 0);
    if (rc) return rc;
    double* acc = e->dsc() + 1;
    e->acc_clean = false;
    HIPCHK(e, hipMemsetAsync(acc, 0, sizeof(double), e->stream));
    hipLaunchKernelGGL(k_eval_u, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, e->ph, e->base_norm, d_x, e->aux.O, e->aux.u,
                       acc, n, e->aux.ld);
    hipLaunchKernelGGL(k_eval_finish, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, e->aux.u, acc, dx, abs_flag, d_u, d_dens,
                       n, e->aux.ld, e->nd.n_out);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}


// ---- observables of the current state (gpe_observe.h) --------------------------------------------------------------------
// every entry point of this section exists once per kind of record, and refuses the engine of the other kind; other: its counterpart
static int obs_wrong_kind(gpe_engine* e, const char* who, const char* other) {
    if (e->cfg.mixture) FAIL(e, GPE_ERR_STATE, "%s: its records are struct gpe_observables, which a mixture engine does not have (%s)", who, other);
    FAIL(e, GPE_ERR_STATE, "%s: not a mixture engine (gpe_config.mixture; a scalar engine has %s)", who, other);
}
static int obs_ensure(gpe_engine* e) {
    if (e->obs_buf) return GPE_OK;
    int rc;
    if ((rc = dev_alloc(e, (Batch*)nullptr, &e->obs_buf, (size_t)2 * OBS_MAX_WG * e->obs_kind->row + e->obs_kind->row))) return rc;
    return dev_alloc(e, (Batch*)nullptr, &e->obs_out, (size_t)e->obs_kind->rec_doubles);
}
// which points an observables call / a monitor may look at: any, unless something exists on the bound points only
static int obs_check_points(gpe_engine* e, const char* who, const float* d_x, int64_t n, const float* d_V) {
    if (n <= 0) FAIL(e, GPE_ERR_INVALID, "%s: need n > 0 points", who);
    if (precomputed_base(e)) {
        if (!(d_x == e->ux && n == e->n_pde))
            FAIL(e, GPE_ERR_INVALID, "%s needs an analytic base on other points than the bound ones (the precomputed base exists on the bound points only)", who);
        if (!e->orth_host[4] || !e->orth_host[5] || !e->orth_host[6]) FAIL(e, GPE_ERR_STATE, "%s: precomputed base not bound (gpe_bind_base)", who);
    }
    if (e->cfg.potential == GPE_POT_PRECOMPUTED && !d_V && !e->pot.on())      // (with terms bound the engine evaluates V on the set itself)
        FAIL(e, GPE_ERR_INVALID, "%s: precomputed potential requested but d_V is NULL", who);
    return GPE_OK;
}
// The chain of kind K (ObsScalar, ObsMix): the two reduction passes over the full jets b.O of the points x, and the record into *dst
// (device memory); nothing synchronises.  q: per-point quadrature weights [n] (the bound set under gpe_bind_weights), or NULL.
extern "C++" {      // (a template inside the C-linkage block of the entry points)
template <class K>
static void obs_chain(gpe_engine* e, const typename K::Arg& ka, Batch& b, const float* x, int64_t n, const float* V, float dv, double* dst,
                      const float* q) {
    const unsigned g = (unsigned)std::min<int64_t>(cdiv(n, OBS_THREADS), OBS_MAX_WG);        // a function of n alone: fixed point -> thread map
    double* slab1 = e->obs_buf;
    double* slab2 = slab1 + (size_t)OBS_MAX_WG * K::ROW;
    double* raw = slab2 + (size_t)OBS_MAX_WG * K::ROW;
    const float* const* bp = (const float* const*)e->orth_dev;
#define OBS_CHAIN(DD, WW)                                                                                                                 \
    hipLaunchKernelGGL((k_obs_pass1<K, DD, WW>), dim3(g), dim3(OBS_THREADS), 0, e->stream, e->ph, e->base_norm, x, V, (const float*)b.O, bp, n, b.ld, slab1, q); \
    hipLaunchKernelGGL(k_obs_reduce<K>, dim3(1), dim3(OBS_THREADS), 0, e->stream, (const double*)slab1, (int)g, raw);                    \
    hipLaunchKernelGGL((k_obs_pass2<K, DD, WW>), dim3(g), dim3(OBS_THREADS), 0, e->stream, e->ph, ka, e->base_norm, x, V, (const float*)b.O, bp, n, b.ld, \
                       (const double*)raw, (double)dv, slab2, q);
    switch (e->nd.dim * 2 + (q ? 1 : 0)) {
        case 2: OBS_CHAIN(1, false) break;
        case 3: OBS_CHAIN(1, true) break;
        case 4: OBS_CHAIN(2, false) break;
        case 5: OBS_CHAIN(2, true) break;
        case 6: OBS_CHAIN(3, false) break;
        default: OBS_CHAIN(3, true) break;
    }
#undef OBS_CHAIN
    hipLaunchKernelGGL(k_obs_finish<K>, dim3(1), dim3(OBS_THREADS), 0, e->stream, e->ph, ka, (const double*)slab2, (int)g, (const double*)raw, (double)dv,
                       (double)n, (const OptDev*)e->od, (typename K::Record*)dst);
}
}
// a mixture's couplings and target norms are those in force now (e->oc.mix, by value)
static int launch_observe(gpe_engine* e, Batch& b, const float* x, int64_t n, const float* V, float dv, double* dst, const float* q = nullptr) {
    if (e->cfg.mixture) obs_chain<ObsMix>(e, e->oc.mix, b, x, n, V, dv, dst, q);
    else obs_chain<ObsScalar>(e, ObsNoArg{}, b, x, n, V, dv, dst, q);
    HIPCHK(e, hipGetLastError());
    return GPE_OK;
}

// gpe_observables / gpe_mixture_observables: out takes one record of the engine's kind
static int observables_impl(gpe_engine* e, const char* who, const float* d_x, int64_t n, const float* d_V, float dv, void* out) {
    const float* q = nullptr;
    if (!d_x) {
        if (!e->ux) FAIL(e, GPE_ERR_STATE, "%s of the bound points before bind_points", who);
        d_x = e->ux; n = e->n_pde; d_V = e->uV;
        q = e->wq;                               // the bound set carries its bound weights; an explicit set and the monitor have none
    }
    int rc;
    if ((rc = obs_check_points(e, who, d_x, n, d_V))) return rc;
    if ((rc = obs_ensure(e))) return rc;
    if (pot_serves(e) && !d_V) {                 // potential terms on a set the engine holds no V for: a scratch V, filled here
        if (e->pot.nVtmp < n) {
            HIPCHK(e, hipStreamSynchronize(e->stream));
            if ((rc = pot_reserve(e, who, &e->pot.Vtmp, &e->pot.nVtmp, n))) return rc;
        }
        if ((rc = pot_fill(e, d_x, n, e->pot.Vtmp))) return rc;
        d_V = e->pot.Vtmp;
    }
    if ((rc = aux_forward(e, d_x, n, 1 + 2 * e->nd.dim, e->nd.dim))) return rc;       // full diagonal second derivatives, as gpe_forward_jets
    if ((rc = launch_observe(e, e->aux, d_x, n, d_V, dv, e->obs_out, q))) return rc;
    HIPCHK(e, hipMemcpyAsync(out, e->obs_out, (size_t)e->obs_kind->rec_doubles * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}
int gpe_observables(gpe_engine* e, const float* d_x, int64_t n, const float* d_V, float dv, struct gpe_observables* out) {
    if (!e || !out) return GPE_ERR_INVALID;
    if (e->cfg.mixture) return obs_wrong_kind(e, "observables", "gpe_mixture_observables");
    return observables_impl(e, "observables", d_x, n, d_V, dv, out);
}
int gpe_mixture_observables(gpe_engine* e, const float* d_x, int64_t n, const float* d_V, float dv, struct gpe_mixture_observables* out) {
    if (!e || !out) return GPE_ERR_INVALID;
    if (!e->cfg.mixture) return obs_wrong_kind(e, "mixture_observables", "gpe_observables");
    return observables_impl(e, "mixture_observables", d_x, n, d_V, dv, out);
}

// ---- keeper: model selection and a patience stop driven by the monitor (gpe_observe.h: k_keep_decide, k_keep_copy) -----------------------
static void keeper_free(gpe_engine* e) {              // the stream is idle, or hipFree waits for it
    if (e->keep.theta_best) (void)hipFree(e->keep.theta_best);
    if (e->keep.dev) (void)hipFree(e->keep.dev);
    e->keep = gpe_engine::Keeper();
}
// "nothing kept": best = +inf, every counter and flag zero
static int keeper_reset(gpe_engine* e, KeepDev* kd) {
    KeepDev h;
    memset(&h, 0, sizeof h);
    h.best = INFINITY;
    HIPCHK(e, hipMemcpyAsync(kd, &h, sizeof h, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}
static int keeper_state(gpe_engine* e, const char* who, KeepDev* h) {      // synchronises
    if (!e->keep.armed()) FAIL(e, GPE_ERR_STATE, "%s: no keeper bound (gpe_bind_keeper)", who);
    return record_copy(e, h, (const KeepDev*)e->keep.dev, hipMemcpyDeviceToHost);
}

static void monitor_free(gpe_engine* e) {
    keeper_free(e);                                   // its metric exists on the monitor's points only
    free_batch(e->mon.b);
    if (e->mon.ring) (void)hipFree(e->mon.ring);
    if (e->mon.Vown) (void)hipFree(e->mon.Vown);
    e->mon = gpe_engine::Monitor();
}

// gpe_bind_monitor / gpe_mixture_monitor: the ring holds records of the engine's kind
static int monitor_bind(gpe_engine* e, const float* d_x, int64_t n, const float* d_V, float dv, int64_t every, int32_t capacity) {
    gpe_engine::Monitor& mn = e->mon;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (!d_x || every <= 0) { monitor_free(e); return GPE_OK; }
    // validate and allocate first, swap last: a bind that fails leaves the monitor that was there, records included
    int rc;
    if ((rc = obs_check_points(e, "monitor", d_x, n, d_V))) return rc;
    if ((rc = obs_ensure(e))) return rc;
    const int cap = capacity > 0 ? capacity : 4096;
    const size_t rec_bytes = (size_t)e->obs_kind->rec_doubles * sizeof(double);
    double* ring = mn.ring;
    if (cap != mn.cap) {
        ring = nullptr;
        if (hipMalloc((void**)&ring, (size_t)cap * rec_bytes) != hipSuccess) {
            (void)hipGetLastError();
            FAIL(e, GPE_ERR_NOMEM, "monitor: no memory for a ring of %d records", cap);
        }
    }
    float* vown = nullptr;                                           // potential terms, no caller array: the engine's own V of this set
    if (pot_serves(e) && !d_V) {
        if (hipMalloc((void**)&vown, (size_t)n * sizeof(float) + 256) != hipSuccess) {
            (void)hipGetLastError();
            if (ring != mn.ring) (void)hipFree(ring);
            FAIL(e, GPE_ERR_NOMEM, "monitor: no memory for the potential on %lld points", (long long)n);
        }
        if ((rc = pot_fill(e, d_x, n, vown))) {                      // filled here, before the monitor changes, and at every change of the terms
            (void)hipFree(vown);
            if (ring != mn.ring) (void)hipFree(ring);
            return rc;
        }
        d_V = vown;
    }
    Batch nb;
    if (mn.b.n == n && mn.b.O) std::swap(nb, mn.b);                 // same size: the batch is reused
    if ((rc = setup_batch(e, nb, d_x, n, 1 + 2 * e->nd.dim, e->nd.dim, false, d_V, /*with_store=*/false))) {
        free_batch(nb);
        if (ring != mn.ring) (void)hipFree(ring);
        if (vown) (void)hipFree(vown);
        return rc;                                                   // (a reused batch cannot fail: nothing is allocated for it)
    }
    free_batch(mn.b);
    mn.b = nb;
    if (ring != mn.ring) { if (mn.ring) (void)hipFree(mn.ring); mn.ring = ring; mn.cap = cap; }
    if (mn.Vown) (void)hipFree(mn.Vown);                             // (the stream is idle)
    mn.Vown = vown;
    HIPCHK(e, hipMemsetAsync(mn.ring, 0, (size_t)cap * rec_bytes, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    mn.x = d_x; mn.V = d_V; mn.n = n; mn.dv = dv; mn.every = every;
    mn.steps = 0; mn.records = 0;
    // an armed keeper stays armed and starts again from "nothing kept": its metric is comparable on one point set only
    if (e->keep.armed()) return keeper_reset(e, e->keep.dev);
    return GPE_OK;
}
// (a clearing call is served whatever the kind: there is nothing of the other kind to clear)
int gpe_bind_monitor(gpe_engine* e, const float* d_x, int64_t n, const float* d_V, float dv, int64_t every, int32_t capacity) {
    if (!e) return GPE_ERR_INVALID;
    if (e->cfg.mixture && d_x && every > 0) return obs_wrong_kind(e, "monitor", "gpe_mixture_monitor");
    return monitor_bind(e, d_x, n, d_V, dv, every, capacity);
}
int gpe_mixture_monitor(gpe_engine* e, const float* d_x, int64_t n, const float* d_V, float dv, int64_t every, int32_t capacity) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->cfg.mixture) return obs_wrong_kind(e, "mixture_monitor", "gpe_bind_monitor");
    return monitor_bind(e, d_x, n, d_V, dv, every, capacity);
}

// ---- analytic potential terms: the entry points (gpe_potential.h) -------------------------------------------------------------------------
int gpe_potential_terms(gpe_engine* e, const gpe_pot_term* terms, int32_t n_terms) {
    if (!e) return GPE_ERR_INVALID;
    if (e->cfg.potential != GPE_POT_PRECOMPUTED)
        FAIL(e, GPE_ERR_INVALID, "potential_terms: the engine's potential is not GPE_POT_PRECOMPUTED (the terms fill the array that path reads)");
    if (!terms) {                                // clear
        if (!e->pot.on()) return GPE_OK;
        if (e->smp.bound()) FAIL(e, GPE_ERR_STATE, "potential_terms: a sampler is bound, and its sets take their potential from the terms (clear the sampler first)");
        if (e->mon.Vown) FAIL(e, GPE_ERR_STATE, "potential_terms: the monitor's potential is evaluated from the terms (clear the monitor first)");
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (e->side) HIPCHK(e, hipStreamSynchronize(e->side));
        const bool unbind = e->pot_bound();
        e->pot.n = 0;
        return unbind ? unbind_points(e) : GPE_OK;
    }
    std::string msg;
    if (int rc = potential_terms_check(terms, n_terms, e->nd.dim, &msg)) { e->err = msg; return rc; }
    e->pot.tab = PotTable{};
    for (int j = 0; j < n_terms; ++j) e->pot.tab.t[j] = terms[j];
    e->pot.n = n_terms;
    // a live engine: the sets whose V the engine owns, in stream order -- no synchronisation, no pointer moves, a captured graph stays valid
    int rc;
    if (e->pot_bound() && (rc = pot_fill(e, e->ux, e->n_pde, e->pot.V))) return rc;
    if (e->mon.Vown && (rc = pot_fill(e, e->mon.x, e->mon.n, e->mon.Vown))) return rc;
    return GPE_OK;
}

int gpe_potential_terms_read(gpe_engine* e, gpe_pot_term* terms_out, int32_t* n_out) {
    if (!e) return GPE_ERR_INVALID;
    if (terms_out) for (int j = 0; j < e->pot.n; ++j) terms_out[j] = e->pot.tab.t[j];
    if (n_out) *n_out = e->pot.n;
    return GPE_OK;
}

int gpe_potential_values(gpe_engine* e, const float** d_V, int64_t* n) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->pot.on()) FAIL(e, GPE_ERR_STATE, "potential_values: no potential terms bound (gpe_potential_terms)");
    if (!e->ux || e->n_pde <= 0) FAIL(e, GPE_ERR_STATE, "potential_values: no points bound");
    if (!e->pot_bound()) FAIL(e, GPE_ERR_STATE, "potential_values: the bound set runs on a caller's array (bound before the terms)");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (d_V) *d_V = e->pot.V;
    if (n) *n = e->n_pde;
    return GPE_OK;
}

int gpe_potential_eval(gpe_engine* e, const float* d_x, int64_t n, float* d_V_out) {
    if (!e) return GPE_ERR_INVALID;
    if (!d_x || !d_V_out || n <= 0) FAIL(e, GPE_ERR_INVALID, "potential_eval: need n > 0 points and an output array");
    if (!e->pot.on()) FAIL(e, GPE_ERR_STATE, "potential_eval: no potential terms bound (gpe_potential_terms)");
    if (int rc = pot_fill(e, d_x, n, d_V_out)) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

// gpe_bind_keeper / gpe_mixture_keeper: the field judged is one of the engine's kind of record (ObsKind)
static int keeper_bind(gpe_engine* e, int metric, double min_delta, int64_t patience) {
    gpe_engine::Keeper& kp = e->keep;
    if (metric == GPE_KEEP_NONE) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        keeper_free(e);
        return GPE_OK;
    }
    // validate and allocate first, swap last: a bind that fails leaves the keeper that was there, its kept set included
    if (metric != GPE_KEEP_RES_RMS && metric != GPE_KEEP_ENERGY) FAIL(e, GPE_ERR_INVALID, "keeper: metric %d is none of GPE_KEEP_RES_RMS, GPE_KEEP_ENERGY", metric);
    if (!e->mon.bound()) FAIL(e, GPE_ERR_INVALID, "keeper: needs a bound monitor (gpe_bind_monitor): it judges the monitor's records");
    if (!(min_delta >= 0.0) || !__builtin_isfinite(min_delta)) FAIL(e, GPE_ERR_INVALID, "keeper: min_delta must be finite and >= 0");
    if (patience < 0) FAIL(e, GPE_ERR_INVALID, "keeper: patience must be >= 0 (0: never stop)");
    if (e->dp.on())
        FAIL(e, GPE_ERR_INVALID, "keeper: this engine has a communicator (gpe_comm_init): every rank's monitor sees its own points, so the ranks would keep "
                                 "and stop at different records; data-parallel keepers are not supported");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    float* tb = kp.theta_best; KeepDev* kd = kp.dev;                  // an armed keeper's buffers are reused (P never changes)
    if (!tb && hipMalloc((void**)&tb, (size_t)e->P * 4 + 256) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(e, GPE_ERR_NOMEM, "keeper: no memory for a copy of %d parameters", e->P);
    }
    if (!kd && hipMalloc((void**)&kd, sizeof(KeepDev)) != hipSuccess) {
        (void)hipGetLastError();
        if (tb != kp.theta_best) (void)hipFree(tb);
        FAIL(e, GPE_ERR_NOMEM, "keeper: no memory for its state");
    }
    int rc = keeper_reset(e, kd);
    if (rc) {                                                         // (an armed keeper may have lost its counters; its buffers stay)
        if (tb != kp.theta_best) (void)hipFree(tb);
        if (kd != kp.dev) (void)hipFree(kd);
        return rc;
    }
    kp.theta_best = tb; kp.dev = kd;
    kp.metric = metric; kp.min_delta = min_delta; kp.patience = patience;
    return GPE_OK;
}
int gpe_bind_keeper(gpe_engine* e, int metric, double min_delta, int64_t patience) {
    if (!e) return GPE_ERR_INVALID;
    if (e->cfg.mixture && metric != GPE_KEEP_NONE) return obs_wrong_kind(e, "keeper", "gpe_mixture_keeper");
    return keeper_bind(e, metric, min_delta, patience);
}
int gpe_mixture_keeper(gpe_engine* e, int metric, double min_delta, int64_t patience) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->cfg.mixture) return obs_wrong_kind(e, "mixture_keeper", "gpe_bind_keeper");
    return keeper_bind(e, metric, min_delta, patience);
}

// gpe_keeper_read / gpe_mixture_keeper_read: rec takes the kept record, one of the engine's kind
static int keeper_read(gpe_engine* e, float* h_flat, size_t n, void* rec, int64_t* seen, int64_t* kept, int64_t* since_best, int* stopped) {
    if (h_flat && (int64_t)n != e->P_user) FAIL(e, GPE_ERR_INVALID, "keeper_read: got %zu floats, model has %d", n, e->P_user);
    KeepDev h;
    int rc;
    if ((rc = keeper_state(e, "keeper_read", &h))) return rc;
    if (seen) *seen = h.seen;
    if (kept) *kept = h.kept;
    if (since_best) *since_best = h.since_best;
    if (stopped) *stopped = h.stopped;
    if (!h_flat && !rec) return GPE_OK;
    if (h.kept == 0) FAIL(e, GPE_ERR_INVALID, "keeper_read: nothing kept yet (%lld records judged, none finite)", (long long)h.seen);
    if (rec) memcpy(rec, h.rec, (size_t)e->obs_kind->rec_doubles * sizeof(double));
    if (h_flat) {
        if ((rc = flat_from_device(e, e->keep.theta_best, h_flat))) return rc;
        HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    return GPE_OK;
}
// (the counters and the parameters are served whatever the kind: only a record has one)
int gpe_keeper_read(gpe_engine* e, float* h_flat, size_t n, struct gpe_observables* rec, int64_t* seen, int64_t* kept, int64_t* since_best, int* stopped) {
    if (!e) return GPE_ERR_INVALID;
    if (e->cfg.mixture && rec) return obs_wrong_kind(e, "keeper_read", "gpe_mixture_keeper_read");
    return keeper_read(e, h_flat, n, rec, seen, kept, since_best, stopped);
}
int gpe_mixture_keeper_read(gpe_engine* e, float* h_flat, size_t n, struct gpe_mixture_observables* rec, int64_t* seen, int64_t* kept,
                            int64_t* since_best, int* stopped) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->cfg.mixture) return obs_wrong_kind(e, "mixture_keeper_read", "gpe_keeper_read");
    return keeper_read(e, h_flat, n, rec, seen, kept, since_best, stopped);
}

int gpe_keeper_restore(gpe_engine* e) {
    if (!e) return GPE_ERR_INVALID;
    KeepDev h;
    int rc;
    if ((rc = keeper_state(e, "keeper_restore", &h))) return rc;
    if (h.kept == 0) FAIL(e, GPE_ERR_INVALID, "keeper_restore: nothing kept yet");
    HIPCHK(e, hipMemcpyAsync(e->theta, e->keep.theta_best, (size_t)e->P * 4, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->packed_dirty = true;                           // as gpe_set_params: the packed weight copies are rebuilt before their next use
    return lbfgs_reset(e);
}

// The monitor's one cadence: k steps (or ticks of gpe_lbfgs_run) were just enqueued -- never past a monitor step: gpe_run cuts its
// replays at Monitor::room() -- and the answer is whether a record is due now.
static bool monitor_tick(gpe_engine* e, int64_t k) {
    if (!e->mon.bound()) return false;
    e->mon.steps += k;
    return e->mon.steps % e->mon.every == 0;
}
// The chain of one record, of theta as it stands (gpe_lbfgs_run puts the judged point there first: lbfgs_monitor_tick): forward of the
// monitor points with the parameters the last step left behind -- on the fused path through the packed weight copies the update
// refreshed, or ensure_packed refreshes here, the path gpe_forward between two gpe_run calls takes -- the reduction chain, one record
// into the ring.
static int monitor_record(gpe_engine* e) {
    gpe_engine::Monitor& mn = e->mon;
    const gpe_engine::Keeper& kp = e->keep;
    int rc;
    if ((rc = mlp_forward(e, mn.b, false))) return rc;
    double* slot = mn.ring + (size_t)(mn.records % mn.cap) * e->obs_kind->rec_doubles;
    if ((rc = launch_observe(e, mn.b, mn.x, mn.n, mn.V, mn.dv, slot))) return rc;
    if (kp.armed()) {                                 // the record just written, judged and -- if it is the best so far -- theta set aside
        hipLaunchKernelGGL(k_keep_decide, dim3(1), dim3(64), 0, e->stream, (const double*)slot,
                           kp.metric == GPE_KEEP_ENERGY ? e->obs_kind->f_energy : e->obs_kind->f_res, e->obs_kind->rec_doubles, kp.min_delta,
                           (long long)kp.patience, kp.dev, e->od);
        const unsigned g = (unsigned)std::min<int64_t>(cdiv((int64_t)cdiv(e->P, 4), KEEP_THREADS), KEEP_MAX_WG);       // a function of P alone
        hipLaunchKernelGGL(k_keep_copy, dim3(g), dim3(KEEP_THREADS), 0, e->stream, (const KeepDev*)kp.dev, (const float*)e->theta, kp.theta_best, e->P);
        HIPCHK(e, hipGetLastError());
    }
    mn.records++;
    return GPE_OK;
}
static int monitor_after_steps(gpe_engine* e, int64_t k) { return monitor_tick(e, k) ? monitor_record(e) : GPE_OK; }

// gpe_read_monitor / gpe_mixture_monitor_read: out takes records of the engine's kind
static int monitor_read(gpe_engine* e, int64_t first, int64_t count, void* out, int64_t* available) {
    const gpe_engine::Monitor& mn = e->mon;
    const size_t rec_bytes = (size_t)e->obs_kind->rec_doubles * sizeof(double);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (available) *available = mn.records;
    if (count == 0) return GPE_OK;
    if (first + count > mn.records)
        FAIL(e, GPE_ERR_INVALID, "monitor records [%lld, %lld) requested, %lld exist", (long long)first, (long long)(first + count), (long long)mn.records);
    if (first < mn.records - mn.cap)
        FAIL(e, GPE_ERR_INVALID, "monitor record %lld is gone: the ring keeps the newest %d of %lld", (long long)first, mn.cap, (long long)mn.records);
    for (int64_t i = 0; i < count;) {
        const int64_t slot = (first + i) % mn.cap;
        const int64_t run = std::min<int64_t>(count - i, mn.cap - slot);
        HIPCHK(e, hipMemcpy((char*)out + i * rec_bytes, (const char*)mn.ring + slot * rec_bytes, run * rec_bytes, hipMemcpyDeviceToHost));
        i += run;
    }
    return GPE_OK;
}
int gpe_read_monitor(gpe_engine* e, int64_t first, int64_t count, struct gpe_observables* out, int64_t* available) {
    if (!e || first < 0 || count < 0 || (count > 0 && !out)) return GPE_ERR_INVALID;
    if (e->cfg.mixture && count == 0) {               // (a mixture engine never held a record of this kind: none available, none to read)
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (available) *available = 0;
        return GPE_OK;
    }
    if (e->cfg.mixture) return obs_wrong_kind(e, "read_monitor", "gpe_mixture_monitor_read");
    return monitor_read(e, first, count, out, available);
}
int gpe_mixture_monitor_read(gpe_engine* e, int64_t first, int64_t count, struct gpe_mixture_observables* out, int64_t* available) {
    if (!e || first < 0 || count < 0 || (count > 0 && !out)) return GPE_ERR_INVALID;
    if (!e->cfg.mixture) return obs_wrong_kind(e, "mixture_monitor_read", "gpe_read_monitor");
    return monitor_read(e, first, count, out, available);
}

// ---- the step ------------------------------------------------------------------------------------------
static unsigned head_grid(gpe_engine* e, int64_t n, int threads = 0) {
    return (unsigned)std::min<int64_t>(cdiv(n, threads > 0 ? threads : e->head_threads), (int64_t)e->num_cu * e->head_wg_per_cu);
}

// energy: a mixture's EN instance, whatever its weight (gpe_mixture_energy)
static int launch_head_pde(gpe_engine* e, bool energy) {
    Batch& b = e->main;
    dim3 g(head_grid(e, b.n));
    const float* none = nullptr;
    if (e->cfg.mixture && (energy || e->mix_wE != 0.f)) {
        if (e->wq) {
            if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_head_mix<CC, EE, true, true>), g, dim3(e->head_threads), 0, e->stream, e->ph, e->oc.mix, b.pts, b.V, b.O, b.u, b.Hu,
                                                e->sums(), b.n, b.ld, e->n_pde, e->bc_target, b.Ob, e->lsums(), e->wq, b.ux); })) return rc;
        } else {
            if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_head_mix<CC, EE, false, true>), g, dim3(e->head_threads), 0, e->stream, e->ph, e->oc.mix, b.pts, b.V, b.O, b.u, b.Hu,
                                                e->sums(), b.n, b.ld, e->n_pde, e->bc_target, b.Ob, e->lsums(), none, b.ux); })) return rc;
        }
    } else
    if (e->cfg.mixture) {
        if (e->wq) {
            if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_head_mix<CC, EE, true>), g, dim3(e->head_threads), 0, e->stream, e->ph, e->oc.mix, b.pts, b.V, b.O, b.u, b.Hu,
                                                e->sums(), b.n, b.ld, e->n_pde, e->bc_target, b.Ob, e->lsums(), e->wq, (float*)nullptr); })) return rc;
        } else {
            if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_head_mix<CC, EE>), g, dim3(e->head_threads), 0, e->stream, e->ph, e->oc.mix, b.pts, b.V, b.O, b.u, b.Hu,
                                                e->sums(), b.n, b.ld, e->n_pde, e->bc_target, b.Ob, e->lsums(), none, (float*)nullptr); })) return rc;
        }
    } else
    if (e->wq) {      // bound quadrature weights: the weighted instance
        if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_head_pde<CC, EE, true>), g, dim3(e->head_threads), 0, e->stream, e->ph, e->base_norm, b.pts, b.V, b.O,
                                            (const float* const*)e->orth_dev, b.u, b.Hu, b.ux, e->sums(), b.n, b.ld, e->n_pde,
                                            e->bc_target, b.Ob, e->lsums(), e->wq); })) return rc;
    } else {
        if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_head_pde<CC, EE>), g, dim3(e->head_threads), 0, e->stream, e->ph, e->base_norm, b.pts, b.V, b.O,
                                            (const float* const*)e->orth_dev, b.u, b.Hu, b.ux, e->sums(), b.n, b.ld, e->n_pde,
                                            e->bc_target, b.Ob, e->lsums(), none); })) return rc;
    }
    HIPCHK(e, hipGetLastError());
    return GPE_OK;
}
// head_slots: the forward pass left that many head triples (StepState::head_slots), which this kernel adds into the sums; 0: k_head_pde did
static int launch_seed_pde(gpe_engine* e, float* d_resid, int want_seeds, int head_slots) {
    Batch& b = e->main;
    dim3 g(head_grid(e, e->n_pde));
    const float* none = nullptr;
    if (e->cfg.mixture && e->mix_wE != 0.f && want_seeds) {      // the seeds of the energy term ride in the EN instance
        if (e->wq) {
            if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_seed_mix<CC, EE, true, true>), g, dim3(e->head_threads), 0, e->stream, e->ph, e->oc.mix, b.pts, b.V, b.u, b.Hu,
                                                e->sums(), b.Ob, d_resid, e->dsc(), e->n_pde, b.ld, want_seeds, e->wq, (const float*)b.ux); })) return rc;
        } else {
            if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_seed_mix<CC, EE, false, true>), g, dim3(e->head_threads), 0, e->stream, e->ph, e->oc.mix, b.pts, b.V, b.u, b.Hu,
                                                e->sums(), b.Ob, d_resid, e->dsc(), e->n_pde, b.ld, want_seeds, none, (const float*)b.ux); })) return rc;
        }
    } else
    if (e->cfg.mixture) {      // (head_slots is 0: a mixture's head never rides in the forward kernel)
        if (e->wq) {
            if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_seed_mix<CC, EE, true>), g, dim3(e->head_threads), 0, e->stream, e->ph, e->oc.mix, b.pts, b.V, b.u, b.Hu,
                                                e->sums(), b.Ob, d_resid, e->dsc(), e->n_pde, b.ld, want_seeds, e->wq, none); })) return rc;
        } else {
            if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_seed_mix<CC, EE>), g, dim3(e->head_threads), 0, e->stream, e->ph, e->oc.mix, b.pts, b.V, b.u, b.Hu,
                                                e->sums(), b.Ob, d_resid, e->dsc(), e->n_pde, b.ld, want_seeds, none, none); })) return rc;
        }
    } else
    if (e->wq) {      // bound quadrature weights: the weighted instance (the head never rode in the forward kernel: head_class)
        if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_seed_pde<CC, EE, true>), g, dim3(e->head_threads), 0, e->stream, e->ph, b.pts, b.V,
                                            (const float* const*)e->orth_dev, b.u, b.Hu, b.ux, e->sums(), b.Ob, d_resid, e->dsc(),
                                            e->n_pde, b.ld, want_seeds, head_slots ? (const double*)e->head_slots : (const double*)nullptr,
                                            head_slots, e->sums(), e->lsums(), e->wq); })) return rc;
    } else {
        if (int rc = launch_ce(e, b, ce_train{}, [&](auto CC, auto EE) { hipLaunchKernelGGL((k_seed_pde<CC, EE>), g, dim3(e->head_threads), 0, e->stream, e->ph, b.pts, b.V,
                                            (const float* const*)e->orth_dev, b.u, b.Hu, b.ux, e->sums(), b.Ob, d_resid, e->dsc(),
                                            e->n_pde, b.ld, want_seeds, head_slots ? (const double*)e->head_slots : (const double*)nullptr,
                                            head_slots, e->sums(), e->lsums(), none); })) return rc;      // collocation rows only; boundary rows were seeded by the head kernel
    }
    HIPCHK(e, hipGetLastError());
    return GPE_OK;
}

static int launch_head_sym(gpe_engine* e) {
    hipLaunchKernelGGL(k_head_sym, dim3(cdiv(e->n_pde, 256)), dim3(256), 0, e->stream, e->ph, e->sym.O, e->sums(), e->n_pde, e->sym.ld);
    if (hipGetLastError() != hipSuccess) FAIL(e, GPE_ERR_HIP, "k_head_sym launch failed");
    return GPE_OK;
}

static int bc_fork(gpe_engine* e, bool with_backward);
static int step_begin(gpe_engine* e, StepOpts o) {
    if (e->main.n <= 0) FAIL(e, GPE_ERR_STATE, "step before bind_points");
    if (precomputed_base(e) && !e->orth_host[4])
        FAIL(e, GPE_ERR_STATE, "precomputed base requested but gpe_bind_base was not called");
    int rc;
    e->st = StepState{};
    StepScope seq{e};
    if ((rc = sampler_before_step(e, o.capturing))) return rc;
    if ((rc = launch_begin(e))) return rc;
    if ((rc = bc_fork(e, true))) return rc;
    // the head rides in the forward kernel, one triple per workgroup of that launch
    const int slots = o.head_may_fuse && head_fusable(e) ? (int)fwd_grid(e, e->main, head_fusable_coop(e)) : 0;
    rc = mlp_forward(e, e->main, true, nullptr, slots);
    if (!rc && !slots) rc = launch_head_pde(e);
    if (!rc && e->cfg.w_sym != 0.f) {
        if (!(rc = mlp_forward(e, e->sym, true))) rc = launch_head_sym(e);
    }
    if (rc) return rc;
    e->st.phase = 1; e->st.head_slots = slots;
    if (e->smp.bound() && !o.capturing) e->smp.steps++;
    return seq.keep();
}
int gpe_step_begin(gpe_engine* e) { return e ? step_begin(e, StepOpts{}) : GPE_ERR_INVALID; }

// Boundary batch (refine/harmonic_pinn_simulation.py:197-210): forward, loss + seeds, reverse.  It does not depend on mu, so it
// is forked onto the side stream at the start of the step and overlaps the collocation batch; its gradient lands in grad_bc
// and k_tail adds it after the join.
static int bc_fork(gpe_engine* e, bool with_backward) {
    e->st.bc_inflight = false;
    if (e->bc.n <= 0 || e->cfg.w_bc == 0.f) return GPE_OK;
    int rc = ensure_packed(e);
    if (rc) return rc;
    if (e->side) {
        HIPCHK(e, hipEventRecord(e->ev_fork, e->stream));
        HIPCHK(e, hipStreamWaitEvent(e->side, e->ev_fork, 0));
    }
    {
        Redirect to_side(e, e->side ? e->side : e->stream, e->grad_bc, e->gslab_bc ? e->gslab_bc : e->gslab);
        if ((rc = mlp_forward(e, e->bc, true))) return rc;
        hipLaunchKernelGGL(k_head_seed_bc, dim3(cdiv(e->bc.n, 256)), dim3(256), 0, e->stream, e->ph, e->base_norm, e->bc.pts.a,
                           e->bc_target, e->bc.O, e->bc.Ob, e->lsums(), e->bc.n, e->bc.ld);
        HIPCHK(e, hipGetLastError());
        if (with_backward && (rc = mlp_backward(e, e->bc, BwdOpts{}))) return rc;
    }
    if (e->side) HIPCHK(e, hipEventRecord(e->ev_join, e->side));
    e->st.bc_inflight = true;
    return GPE_OK;
}
static int bc_join(gpe_engine* e) {
    if (e->st.bc_inflight && e->side) HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_join, 0));
    return GPE_OK;
}
static int launch_tail(gpe_engine* e, bool add_bc) {
    const float* add = (add_bc && e->st.bc_inflight) ? e->grad_bc : nullptr;
    hipLaunchKernelGGL(k_tail, dim3(add ? cdiv(e->P, 256) : 1), dim3(256), 0, e->stream, e->grad, add, e->P, e->dsc());
    HIPCHK(e, hipGetLastError());
    e->st.bc_inflight = false;
    return GPE_OK;
}

// bucketed: the synchronous data-parallel step all-reduces every finished layer of the generic set behind the remaining reverse pass
static int step_backward(gpe_engine* e, StepOpts o, bool bucketed = false) {
    if (e->st.phase != 1) FAIL(e, GPE_ERR_STATE, "step_backward without step_begin");
    StepScope seq{e};
    int rc = GPE_OK;
    const bool with_sym = e->cfg.w_sym != 0.f;
    // small batches of the common problem class (real psi, no orthogonality / Riesz / symmetry terms) on the pipelined reverse
    // kernel: the seeds are formed inside it
    const BwdOpts bo{/*close=*/!with_sym, /*assign=*/true, seed_in_reverse(e), o.update_may_fuse, bucketed};
    if (!bo.seeds_in_kernel && (rc = launch_seed_pde(e, nullptr, 1, e->st.head_slots))) return rc;
    rc = mlp_backward(e, e->main, bo);
    e->st.head_slots = 0;
    if (rc) return rc;
    if (with_sym) {
        hipLaunchKernelGGL(k_seed_sym, dim3(cdiv(e->n_pde, 256)), dim3(256), 0, e->stream, e->ph, e->sym.O, e->sym.Ob,
                           e->n_pde, e->sym.ld);
        HIPCHK(e, hipGetLastError());
        if ((rc = mlp_backward(e, e->sym, BwdOpts{/*close=*/true, /*assign=*/false}))) return rc;
    }
    e->st.phase = 2;
    return seq.keep();
}
int gpe_step_backward(gpe_engine* e) { return e ? step_backward(e, StepOpts{}) : GPE_ERR_INVALID; }

static void after_update(gpe_engine* e) {          // host-side mirror of what k_update left behind
    e->acc_clean = true;
    e->packed_dirty = e->path == GPE_PATH_FUSED && e->upd_snap != nullptr;      // multi-workgroup update: the next k_begin repacks
}
// the pre-training loss is and stays unweighted: its mean is over the point count whatever gpe_bind_weights published as W
static Phys phys_counted(const gpe_engine* e) { Phys ph = e->ph; ph.n_global = counted_n_global(e); return ph; }
// The update launch and its tail (error check, after_update).  Forms: one workgroup; UPD_G workgroups behind k_update_part (upd_snap); UPD_G
// workgroups on the snapshot the slab reduction left (k_grad_reduce_part, upd_snap_small), new weights scattered into the packed copies
enum UpdForm { UPD_ONE, UPD_MULTI, UPD_PARTS };
static UpdForm update_form(const gpe_engine* e) { return e->upd_snap ? UPD_MULTI : UPD_ONE; }
static int launch_update(gpe_engine* e, UpdForm form, const float* grad, const double* sums, const double* lsums, double bc_cnt, int do_update,
                         int mse_mode, double* dbl_keep) {
    const Phys ph = mse_mode ? phys_counted(e) : e->ph;
    const UpdSnap* snap = form == UPD_ONE ? nullptr : (form == UPD_MULTI ? e->upd_snap : e->upd_snap_small);
    const int pack_mode = form == UPD_ONE ? update_pack_mode(e) : (form == UPD_MULTI ? 1 : 2);
    if (form == UPD_MULTI) hipLaunchKernelGGL(k_update_part, dim3(UPD_G), dim3(1024), 0, e->stream, e->P, grad, sums, lsums, e->od, e->upd_snap);
    hipLaunchKernelGGL(form == UPD_ONE ? k_update<false> : k_update<true>, dim3(form == UPD_ONE ? 1 : UPD_G), dim3(1024), 0, e->stream, e->P, e->theta,
                       e->am, e->av, grad, sums, lsums, ph, e->oc, e->od, e->hist, e->cap, e->last, bc_cnt, do_update, mse_mode, e->nd, e->H, e->Wpk,
                       e->WpkT, pack_count(e), e->dbl, (int)DBL_COUNT, dbl_keep, snap, pack_mode);
    HIPCHK(e, hipGetLastError());
    after_update(e);
    return GPE_OK;
}
static double bc_count(gpe_engine* e) {
    const int64_t nb = e->nb_merged > 0 ? e->nb_merged : e->bc.n;
    return (nb > 0 && e->cfg.w_bc != 0.f) ? (double)nb * e->nd.n_out : 0.0;
}

static int step_update(gpe_engine* e) {
    if (e->st.phase != 2) FAIL(e, GPE_ERR_STATE, "step_update without step_backward");
    StepScope seq{e};               // the step ends here
    if (e->st.update_done) { after_update(e); return GPE_OK; }      // the slab reduction's last workgroup ran it
    return launch_update(e, e->st.update_parts ? UPD_PARTS : update_form(e), e->grad, e->sums(), e->lsums(), bc_count(e), 1, 0, nullptr);
}
int gpe_step_update(gpe_engine* e) { return e ? step_update(e) : GPE_ERR_INVALID; }

// ---- pre-training on an analytic target (refine/harmonic_pinn_simulation.py:650-701) ---------------------------------
int gpe_bind_target(gpe_engine* e, const float* d_target) {
    if (!e) return GPE_ERR_INVALID;
    if (e->main.n <= 0) FAIL(e, GPE_ERR_STATE, "bind_target before bind_points");
    if (e->smp.bound()) FAIL(e, GPE_ERR_STATE, "bind_target: a sampler is bound, a target array would go stale at its next redraw");
    e->mse_target = d_target;
    if (!d_target) { free_batch(e->mse); return GPE_OK; }
    return setup_batch(e, e->mse, e->ux, e->n_pde, 1, 0, false, nullptr);
}

int gpe_mse_begin(gpe_engine* e) {
    if (!e) return GPE_ERR_INVALID;
    if (e->smp.bound()) FAIL(e, GPE_ERR_STATE, "mse step while a sampler is bound: the target lives on fixed points");
    if (!e->mse_target || e->mse.n <= 0) FAIL(e, GPE_ERR_STATE, "mse step before bind_target");
    int rc;
    e->st = StepState{};
    StepScope seq{e};
    e->mse.pts = Pts{e->ux, nullptr, e->n_pde};
    if ((rc = launch_begin(e))) return rc;
    if ((rc = mlp_forward(e, e->mse, true))) return rc;
    hipLaunchKernelGGL(k_seed_mse, dim3(head_grid(e, e->mse.n, 256)), dim3(256), 0, e->stream, phys_counted(e), e->mse.pts.a, e->mse_target,
                       e->mse.O, e->mse.Ob, e->dsc() + 2, e->mse.n, e->mse.ld);
    HIPCHK(e, hipGetLastError());
    if ((rc = mlp_backward(e, e->mse, BwdOpts{/*close=*/true}))) return rc;
    e->st.phase = 3;
    return seq.keep();
}

static int mse_finish(gpe_engine* e, int do_update) {
    if (e->st.phase != 3) FAIL(e, GPE_ERR_STATE, "mse update without mse begin");
    StepScope seq{e};
    // sums[S_DEN] must be non-zero for the (unused) Rayleigh quotient of the shared update kernel
    return launch_update(e, update_form(e), e->grad, e->sums(), e->lsums(), 0.0, do_update, 1, nullptr);
}

int gpe_mse_update(gpe_engine* e) { return e ? mse_finish(e, 1) : GPE_ERR_INVALID; }

int gpe_mse_step(gpe_engine* e, gpe_scalars* out) {
    int rc;
    if ((rc = gpe_mse_begin(e))) return rc;
    if ((rc = mse_finish(e, 1))) return rc;
    if (out) return gpe_read_scalars(e, out);
    return GPE_OK;
}

int gpe_mse_loss_grad(gpe_engine* e, double* loss) {
    int rc;
    if ((rc = gpe_mse_begin(e))) return rc;
    if ((rc = mse_finish(e, 0))) return rc;
    gpe_scalars sc;
    if ((rc = last_record_read(e, &sc))) return rc;
    if (loss) *loss = sc.loss;
    return GPE_OK;
}


// ---- device-resident L-BFGS (gpe_lbfgs.h; torch.optim.LBFGS without a line search, flattened) ---------------------------------------
// One iteration = the evaluation the caller enqueued (gpe_step_begin + gpe_step_backward, or gpe_mse_begin) + the record launch (the
// update kernel with do_update = 0: the loss L-BFGS sees IS the one k_update records, the step sums are consumed, Adam's state is not
// touched) + k_lbfgs_dots, k_lbfgs_coef, k_lbfgs_apply.  Nothing synchronises.  The packed weight copies are refreshed as after the
// multi-workgroup Adam update: the next step's k_begin repacks (packed_dirty).
int gpe_lbfgs_config(gpe_engine* e, double lr, int history, double tolerance_grad, double tolerance_change, double stop_loss) {
    if (!e) return GPE_ERR_INVALID;
    if (history < 1 || history > LBFGS_MAX_HISTORY) FAIL(e, GPE_ERR_INVALID, "lbfgs_config: history must be in [1,%d], got %d", LBFGS_MAX_HISTORY, history);
    if (!(__builtin_isfinite(lr) && lr > 0.0)) FAIL(e, GPE_ERR_INVALID, "lbfgs_config: lr must be finite and positive");
    if (!(__builtin_isfinite(tolerance_grad) && tolerance_grad >= 0.0) || !(__builtin_isfinite(tolerance_change) && tolerance_change >= 0.0) ||
        !(__builtin_isfinite(stop_loss) && stop_loss >= 0.0))
        FAIL(e, GPE_ERR_INVALID, "lbfgs_config: tolerance_grad, tolerance_change and stop_loss must be finite and not negative");
    if (e->cfg.world_size > 1 || e->dp.on()) FAIL(e, GPE_ERR_INVALID, "lbfgs_config: a data-parallel engine has no L-BFGS (the history is per rank)");
    if (!e->lb.st || e->lb.cfg.m != history) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        lbfgs_free_history(e);                        // the line search, gpe_lbfgs_monitor and their buffers do not depend on `history`
        gpe_engine::Lbfgs::Hist& h = e->lb.h;
        const int m = history;
        e->lb.ld = (int)round_up(e->P, 64);
        e->lb.n_part = lbfgs_grid(e->P);
        int rc;
        if ((rc = dev_alloc(e, nullptr, &h.S, (size_t)m * e->lb.ld)) || (rc = dev_alloc(e, nullptr, &h.Y, (size_t)m * e->lb.ld)) ||
            (rc = dev_alloc(e, nullptr, &h.g_prev, (size_t)e->lb.ld)) || (rc = dev_alloc(e, nullptr, &h.d, (size_t)e->lb.ld)) ||
            (rc = dev_alloc(e, nullptr, &h.part, (size_t)e->lb.n_part * lbfgs_row(m))) ||
            (rc = dev_alloc(e, nullptr, &h.SY, (size_t)m * m)) || (rc = dev_alloc(e, nullptr, &h.YY, (size_t)m * m)) ||
            (rc = dev_alloc(e, nullptr, &h.ro, (size_t)m)) || (rc = dev_alloc(e, nullptr, &h.coef, (size_t)2 * m + 1)) ||
            (!e->lb.st && (rc = dev_alloc(e, nullptr, &e->lb.st, (size_t)1)))) { lbfgs_free(e); return rc; }
    }
    e->lb.cfg = LbfgsCfg{lr, tolerance_grad, tolerance_change, stop_loss, history};
    e->lb.on = true;
    return lbfgs_reset(e);
}

// Refuses an engine without L-BFGS; h: the state as the work enqueued so far leaves it, on the host (every reader synchronises here)
static int lbfgs_state(gpe_engine* e, const char* who, LbfgsDev* h = nullptr) {
    if (!e->lb.on) FAIL(e, GPE_ERR_STATE, "%s: L-BFGS is not configured (gpe_lbfgs_config)", who);
    return h ? record_copy(e, h, (const LbfgsDev*)e->lb.st, hipMemcpyDeviceToHost) : GPE_OK;
}

static int lbfgs_refusals(gpe_engine* e, const char* who) {
    int rc;
    if ((rc = lbfgs_state(e, who))) return rc;
    if (e->smp.bound()) FAIL(e, GPE_ERR_STATE, "%s: a sampler with every > 0 is bound, the objective would change under the history", who);
    if (e->dp.on()) FAIL(e, GPE_ERR_STATE, "%s: the engine has a communicator, L-BFGS is single-rank", who);
    return GPE_OK;
}

// the iteration's three launches; LS: on the point the tick's decision accepted, if it accepted one (gpe_lbfgs.h)
extern "C++" template <bool LS>
static void launch_lbfgs_iteration(gpe_engine* e) {
    const gpe_engine::Lbfgs& lb = e->lb;
    const int m = lb.cfg.m;
    hipLaunchKernelGGL(k_lbfgs_dots<LS>, dim3(lb.n_part), dim3(64), 0, e->stream, e->P, lb.ld, m, (const float*)e->grad, (const float*)lb.h.g_prev,
                       (const float*)lb.h.d, (const float*)lb.h.S, (const float*)lb.h.Y, (const LbfgsDev*)lb.st, lb.h.part);
    hipLaunchKernelGGL(k_lbfgs_coef<LS>, dim3(1), dim3(256), 0, e->stream, m, lb.n_part, lb.cfg, lb.st, (const double*)lb.h.part, lb.h.SY, lb.h.YY,
                       lb.h.ro, lb.h.coef, (const gpe_scalars*)e->last);
    hipLaunchKernelGGL(k_lbfgs_apply<LS>, dim3(cdiv(e->P, 256)), dim3(256), 0, e->stream, e->P, lb.ld, m, (const float*)e->grad, lb.h.g_prev, lb.h.d,
                       lb.h.S, lb.h.Y, e->theta, (const LbfgsDev*)lb.st, (const double*)lb.h.coef);
}

int gpe_lbfgs_update(gpe_engine* e) {
    if (!e) return GPE_ERR_INVALID;
    int rc;
    if ((rc = lbfgs_refusals(e, "lbfgs_update"))) return rc;
    if (e->st.phase != 2 && e->st.phase != 3) FAIL(e, GPE_ERR_STATE, "lbfgs_update without step_backward or mse_begin");
    const int mse = e->st.phase == 3;
    StepScope seq{e};               // the step ends here
    if ((rc = launch_update(e, update_form(e), e->grad, e->sums(), e->lsums(), mse ? 0.0 : bc_count(e), /*do_update=*/0, mse, nullptr))) return rc;
    if (e->lb.ls.kind) {                                // one tick: the same five launches whatever the decision is
        hipLaunchKernelGGL(k_ls_dots, dim3(e->lb.n_part), dim3(64), 0, e->stream, e->P, e->lb.ld, (const float*)e->grad, (const float*)e->lb.h.d,
                           (const LbfgsDev*)e->lb.st, e->lb.ls_part);
        hipLaunchKernelGGL(k_ls_decide, dim3(1), dim3(64), 0, e->stream, e->lb.n_part, e->lb.cfg, e->lb.ls, e->lb.st, (const double*)e->lb.ls_part,
                           (const gpe_scalars*)e->last);
        launch_lbfgs_iteration<true>(e);
    } else launch_lbfgs_iteration<false>(e);
    HIPCHK(e, hipGetLastError());
    e->packed_dirty = e->path == GPE_PATH_FUSED;      // theta moved behind the record launch's repack: the next k_begin repacks
    return GPE_OK;
}

// gpe_lbfgs_monitor: one tick of gpe_lbfgs_run is one step of the monitor's cadence.  On a monitor tick the judged point (gpe_lbfgs.h)
// stands in theta's place for the length of the monitor chain -- on the fused path mlp_forward repacks the weight copies from it -- and
// theta comes back behind it, so the run goes on from the bits it would have had; the next evaluation repacks, as after every tick.
static int lbfgs_monitor_tick(gpe_engine* e) {
    if (!e->lb.mon || !monitor_tick(e, 1)) return GPE_OK;
    const unsigned g = lbfgs_view_grid(e->P);
    hipLaunchKernelGGL(k_lbfgs_view, dim3(g), dim3(LBV_THREADS), 0, e->stream, e->P, e->theta, e->lb.view_buf, e->lb.st);
    HIPCHK(e, hipGetLastError());
    e->packed_dirty = e->path == GPE_PATH_FUSED;
    const int rc = monitor_record(e);
    hipLaunchKernelGGL(k_lbfgs_unview, dim3(g), dim3(LBV_THREADS), 0, e->stream, e->P, e->theta, (const float*)e->lb.view_buf, e->lb.st,
                       (const KeepDev*)(e->keep.armed() ? e->keep.dev : nullptr));
    HIPCHK(e, hipGetLastError());
    e->packed_dirty = e->path == GPE_PATH_FUSED;
    return rc;
}

int gpe_lbfgs_run(gpe_engine* e, int64_t n_iters, int mse) {
    if (!e || n_iters < 0) return GPE_ERR_INVALID;
    int rc;
    if ((rc = lbfgs_refusals(e, "lbfgs_run"))) return rc;
    for (int64_t i = 0; i < n_iters; ++i) {
        if (mse) rc = gpe_mse_begin(e);
        else if (!(rc = step_begin(e, StepOpts{}))) rc = step_backward(e, StepOpts{});
        if (!rc) rc = gpe_lbfgs_update(e);
        if (!rc) rc = lbfgs_monitor_tick(e);
        if (rc) return rc;
    }
    return GPE_OK;
}

int gpe_lbfgs_monitor(gpe_engine* e, int on) {
    if (!e) return GPE_ERR_INVALID;
    if (on != 0 && on != 1) FAIL(e, GPE_ERR_INVALID, "lbfgs_monitor: on must be 0 or 1, got %d", on);
    int rc;
    if ((rc = lbfgs_state(e, "lbfgs_monitor"))) return rc;
    if (on && !e->lb.view_buf && (rc = dev_alloc(e, nullptr, &e->lb.view_buf, (size_t)e->lb.ld))) return rc;
    e->lb.mon = on != 0;
    return GPE_OK;
}

int gpe_lbfgs_point(gpe_engine* e, float* h_flat, size_t n) {
    if (!e) return GPE_ERR_INVALID;
    if (!h_flat) FAIL(e, GPE_ERR_INVALID, "lbfgs_point: no output array");
    if ((int64_t)n != e->P_user) FAIL(e, GPE_ERR_INVALID, "lbfgs_point: got %zu floats, model has %d", n, e->P_user);
    LbfgsDev h;
    if (int rc = lbfgs_state(e, "lbfgs_point", &h)) return rc;
    // the rule of k_lbfgs_view, on a copy of the state: this reader synchronises anyway, and it writes nothing on the device
    if (int rc = flat_from_device(e, lbfgs_judged_at_start(&h) ? h.ls.theta0 : e->theta, h_flat)) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return GPE_OK;
}

int gpe_lbfgs_read(gpe_engine* e, double out[16]) {
    if (!e || !out) return GPE_ERR_INVALID;
    static_assert(LBR_FIELDS == 16, "gpe_lbfgs_read record");
    LbfgsDev h;
    if (int rc = lbfgs_state(e, "lbfgs_read", &h)) return rc;
    memcpy(out, h.rec, sizeof h.rec);
    // the state as it stands (a reset clears it; the record fields of the last iteration would be stale then)
    out[LBR_N_ITER] = (double)h.n_iter; out[LBR_COUNT] = h.count; out[LBR_FROZEN] = h.frozen; out[LBR_HEAD] = h.head; out[LBR_H_DIAG] = h.H_diag;
    out[LBR_T] = h.t; out[LBR_PREV_LOSS] = h.prev_loss;
    return GPE_OK;
}

int gpe_lbfgs_line_search(gpe_engine* e, int kind, double c1, double c2, int max_ls) {
    if (!e) return GPE_ERR_INVALID;
    if (kind != 0 && kind != 1) FAIL(e, GPE_ERR_INVALID, "lbfgs_line_search: kind must be 0 (none) or 1 (strong Wolfe), got %d", kind);
    if (!(__builtin_isfinite(c1) && __builtin_isfinite(c2))) FAIL(e, GPE_ERR_INVALID, "lbfgs_line_search: c1 and c2 must be finite");
    if (!(0.0 < c1 && c1 < c2 && c2 < 1.0)) FAIL(e, GPE_ERR_INVALID, "lbfgs_line_search: 0 < c1 < c2 < 1 required, got %g, %g", c1, c2);
    if (max_ls < 1 || max_ls > 64) FAIL(e, GPE_ERR_INVALID, "lbfgs_line_search: max_ls must be in [1,64], got %d", max_ls);
    int rc;
    if ((rc = lbfgs_state(e, "lbfgs_line_search"))) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (kind && !e->lb.ls_buf) {
        if ((rc = dev_alloc(e, nullptr, &e->lb.ls_buf, (size_t)(LS_SLOTS + 1) * e->lb.ld)) ||
            (rc = dev_alloc(e, nullptr, &e->lb.ls_part, (size_t)e->lb.n_part * LSD_COUNT))) return rc;
    }
    // a search of the previous setting may be running: theta goes back to its start point before the state is cleared
    rc = lbfgs_reset(e, /*theta_to_start=*/true);
    e->lb.ls = LsCfg{kind, c1, c2, max_ls};
    return rc;
}

int gpe_lbfgs_ls_read(gpe_engine* e, double out[24]) {
    if (!e || !out) return GPE_ERR_INVALID;
    static_assert(LSR_FIELDS == 24, "gpe_lbfgs_ls_read record");
    LbfgsDev h;
    if (int rc = lbfgs_state(e, "lbfgs_ls_read", &h)) return rc;
    const LsDev& ls = h.ls;
    out[LSR_PHASE] = ls.did; out[LSR_LS_ITER] = ls.ls_iter; out[LSR_LS_EVALS] = ls.ls_evals; out[LSR_EVALS_TOTAL] = (double)ls.evals_total;
    out[LSR_T] = ls.t; out[LSR_T_PREV] = ls.state == LS_BRACKET ? ls.b[0] : 0.0;
    out[LSR_B0] = ls.b[0]; out[LSR_B1] = ls.b[1]; out[LSR_BF0] = ls.bf[0]; out[LSR_BF1] = ls.bf[1];
    out[LSR_BGTD0] = ls.bgtd[0]; out[LSR_BGTD1] = ls.bgtd[1]; out[LSR_LOW_POS] = ls.low_pos;
    out[LSR_F0] = ls.f0; out[LSR_GTD0] = ls.gtd0; out[LSR_DNORM] = ls.dnorm;
    out[LSR_ACCEPTED] = (double)ls.accepted; out[LSR_END_MAX_LS] = (double)ls.end_max_ls; out[LSR_END_WIDTH] = (double)ls.end_width;
    out[LSR_END_CURV] = (double)ls.end_curv; out[LSR_STALLED] = (double)ls.stalled; out[LSR_INSUF] = ls.insuf;
    out[LSR_BSLOTS] = ls.bslot[0] + 4 * ls.bslot[1]; out[LSR_SLOT_NEW] = ls.slot_new;
    return GPE_OK;
}

int gpe_lbfgs_history(gpe_engine* e, float* h_S, float* h_Y, float* h_g_prev, float* h_d, size_t n, int* count) {
    if (!e) return GPE_ERR_INVALID;
    LbfgsDev h;
    int rc;
    if ((rc = lbfgs_state(e, "lbfgs_history", &h))) return rc;
    if ((int64_t)n != e->P_user) FAIL(e, GPE_ERR_INVALID, "lbfgs_history: rows of %zu floats, model has %d", n, e->P_user);
    const int m = e->lb.cfg.m;
    for (int a = 0; a < h.count; ++a) {               // age order: row 0 is the oldest pair
        const int j = (h.head - h.count + a + m) % m;
        if (h_S && (rc = flat_from_device(e, e->lb.h.S + (size_t)j * e->lb.ld, h_S + (size_t)a * n))) return rc;
        if (h_Y && (rc = flat_from_device(e, e->lb.h.Y + (size_t)j * e->lb.ld, h_Y + (size_t)a * n))) return rc;
    }
    if (h_g_prev && (rc = flat_from_device(e, e->lb.h.g_prev, h_g_prev))) return rc;
    if (h_d && (rc = flat_from_device(e, e->lb.h.d, h_d))) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (count) *count = h.count;
    return GPE_OK;
}

// ---- data-parallel exchange inside the engine -------------------------------------------------------------------
// One process per GPU.  librccl is dlopen'ed here (the copy already mapped into the process -- PyTorch-ROCm's -- if there is one,
// else ROCm's), so libgpe_hip.so has no link-time dependency on it and single-GPU users never load it.
static int rccl_load(gpe_engine* e) {
    if (e->dp.rccl.dl) return GPE_OK;
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;      // reuse a mapped copy
    if (!h) for (const char* n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) FAIL(e, GPE_ERR_STATE, "librccl.so not found: %s", dlerror());
    e->dp.rccl.dl = h;
    *(void**)&e->dp.rccl.GetUniqueId = dlsym(h, "ncclGetUniqueId");
    *(void**)&e->dp.rccl.CommInitRank = dlsym(h, "ncclCommInitRank");
    *(void**)&e->dp.rccl.CommDestroy = dlsym(h, "ncclCommDestroy");
    *(void**)&e->dp.rccl.AllReduce = dlsym(h, "ncclAllReduce");
    *(void**)&e->dp.rccl.GetErrorString = dlsym(h, "ncclGetErrorString");
    if (!e->dp.rccl.GetUniqueId || !e->dp.rccl.CommInitRank || !e->dp.rccl.CommDestroy || !e->dp.rccl.AllReduce || !e->dp.rccl.GetErrorString) {
        e->dp.rccl.dl = nullptr;
        FAIL(e, GPE_ERR_STATE, "librccl.so lacks a required symbol");
    }
    return GPE_OK;
}
#define RCCLCHK(e, call)                                                                                             \
    do {                                                                                                             \
        ncclResult_t _r = (call);                                                                                    \
        if (_r != ncclSuccess) FAIL(e, GPE_ERR_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #call, (e)->dp.rccl.GetErrorString(_r)); \
    } while (0)

int gpe_comm_unique_id(gpe_engine* e, void* out128) {
    if (!e || !out128) return GPE_ERR_INVALID;
    int rc = rccl_load(e);
    if (rc) return rc;
    static_assert(sizeof(ncclUniqueId) == GPE_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    RCCLCHK(e, e->dp.rccl.GetUniqueId(&id));
    memcpy(out128, &id, sizeof id);
    return GPE_OK;
}

int gpe_comm_init(gpe_engine* e, const void* id128, int rank, int world) {
    if (!e || !id128 || world < 1 || rank < 0 || rank >= world) return GPE_ERR_INVALID;
    if (e->dp.on()) FAIL(e, GPE_ERR_STATE, "communicator already initialised");
    if (e->smp.adaptive()) FAIL(e, GPE_ERR_STATE, "comm_init: an adaptive sampler is bound, and a data-parallel allocation needs a mass exchange");
    if (world != (e->cfg.world_size > 0 ? e->cfg.world_size : 1))
        FAIL(e, GPE_ERR_INVALID, "comm world %d != gpe_config.world_size %d", world, e->cfg.world_size);
    int rc = rccl_load(e);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    RCCLCHK(e, e->dp.rccl.CommInitRank(&e->dp.comm, world, id, rank));
    e->dp.rank = rank; e->dp.world = world;
    e->dp.inline_sync = env_on("GPE_DP_INLINE");
    HIPCHK(e, hipStreamCreateWithFlags(&e->dp.stream, hipStreamNonBlocking));
    HIPCHK(e, hipEventCreateWithFlags(&e->dp.ev_x0, hipEventDisableTiming));
    HIPCHK(e, hipEventCreateWithFlags(&e->dp.ev_x1, hipEventDisableTiming));
    e->dp.ev_bucket.resize(e->nd.n_lin);
    for (auto& ev : e->dp.ev_bucket) HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    e->dp.collectives = 0;
    return GPE_OK;
}

// what gpe_comm_set_async allocated
static void dp_async_free(gpe_engine* e) {
    for (auto& ev : e->dp.ev_g) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
    if (e->dp.grad_alt) { (void)hipFree(e->dp.grad_alt); e->dp.grad_alt = nullptr; }
    if (e->dp.dbl_prev) { (void)hipFree(e->dp.dbl_prev); e->dp.dbl_prev = nullptr; }
    e->dp.async_grad = false;
}

int gpe_comm_destroy(gpe_engine* e) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->dp.on()) return GPE_OK;
    (void)hipStreamSynchronize(e->stream);
    (void)hipStreamSynchronize(e->dp.stream);
    (void)e->dp.rccl.CommDestroy(e->dp.comm);
    e->dp.comm = nullptr;
    (void)hipStreamDestroy(e->dp.stream); e->dp.stream = nullptr;
    (void)hipEventDestroy(e->dp.ev_x0); (void)hipEventDestroy(e->dp.ev_x1); e->dp.ev_x0 = e->dp.ev_x1 = nullptr;
    for (hipEvent_t ev : e->dp.ev_bucket) (void)hipEventDestroy(ev);
    e->dp.ev_bucket.clear();
    dp_async_free(e);
    return GPE_OK;
}

int gpe_comm_info(const gpe_engine* e, int* rank, int* world, int64_t* collectives) {
    if (!e) return GPE_ERR_INVALID;
    if (rank) *rank = e->dp.on() ? e->dp.rank : -1;
    if (world) *world = e->dp.on() ? e->dp.world : 0;
    if (collectives) *collectives = e->dp.collectives;
    return GPE_OK;
}

// all-reduce(sum) buf in place.  behind == NULL: on the compute stream itself; an event: on the exchange stream, once everything enqueued
// on the compute stream so far has finished (the event is recorded there)
static int dp_allreduce(gpe_engine* e, void* buf, size_t count, ncclDataType_t dt, hipEvent_t behind) {
    if (behind) {
        HIPCHK(e, hipEventRecord(behind, e->stream));
        HIPCHK(e, hipStreamWaitEvent(e->dp.stream, behind, 0));
    }
    RCCLCHK(e, e->dp.rccl.AllReduce(buf, buf, count, dt, ncclSum, e->dp.comm, behind ? e->dp.stream : e->stream));
    e->dp.collectives++;
    return GPE_OK;
}
static int dp_join(gpe_engine* e) {       // the compute stream continues after everything on the exchange stream
    HIPCHK(e, hipEventRecord(e->dp.ev_x1, e->dp.stream));
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->dp.ev_x1, 0));
    return GPE_OK;
}
// the exchange of the step sums between the passes: the reverse pass reads the global ones
static int dp_exchange_sums(gpe_engine* e, bool inl) {
    int rc = dp_allreduce(e, e->sums(), S_COUNT, ncclDouble, inl ? nullptr : e->dp.ev_x0);
    return rc || inl ? rc : dp_join(e);
}

// First phase of an engine-driven data-parallel step: as in gpe_step nobody reads the step sums between the passes, so the forward
// kernel may run the head (the N = 1 kernels: no k_head_pde); its per-workgroup triples are added by one small launch into the sums
// the first all-reduce exchanges, and the reverse phase then reads the GLOBAL sums like after k_head_pde.
static int dp_begin(gpe_engine* e) {
    int rc = step_begin(e, StepOpts{/*head_may_fuse=*/true});
    if (rc) return rc;
    if (e->st.head_slots) {
        hipLaunchKernelGGL(k_slots_to_sums, dim3(1), dim3(64), 0, e->stream, (const double*)e->head_slots, e->st.head_slots, e->sums(), e->lsums());
        HIPCHK(e, hipGetLastError());
        e->st.head_slots = 0;                       // consumers take the (all-reduced) sums, not the local slots
    }
    return GPE_OK;
}

// One synchronous data-parallel step, no host synchronisation: begin -> all-reduce of the 12 double sums -> backward with the
// gradient all-reduced on the exchange stream (generic set: one bucket per linear map, output map first, behind the remaining
// reverse pass; fused set: the reverse pass is a single kernel, so one P+4 message) -> clip/Adam (replicated, bit-identical).
// One-step-stale variant (gpe_comm_set_async).  Step t: forward / sums exchange / reverse with theta_t -> g_t; its all-reduce is
// issued on the exchange stream and NOT waited for; the update of step t applies g_{t-1} (all-reduced while step t computed) with
// the scalars of step t-1.  Step 0 applies nothing.  Records (gpe_read_scalars, history) therefore lag one step.
static int step_dp_async(gpe_engine* e) {
    int rc;
    const int cur = (int)(e->dp.async_t & 1), prv = cur ^ 1;
    float* gcur = (e->dp.async_t & 1) ? e->dp.grad_alt : e->grad;       // the two gradient buffers alternate
    e->acc_clean = e->acc_clean && e->path == GPE_PATH_FUSED;
    StepScope seq{e};
    {
        // this step's buffer: zeroed by k_begin (generic set), written by the reverse pass; the other one holds g_{t-1} until this
        // step's update has applied it
        Redirect to_cur(e, e->stream, gcur, e->gslab);
        if ((rc = dp_begin(e))) return rc;
        if ((rc = dp_exchange_sums(e, /*inl=*/false))) return rc;
        if ((rc = step_backward(e, StepOpts{}))) return rc;
        if ((rc = dp_allreduce(e, gcur, (size_t)e->P + GT_COUNT, ncclFloat, e->dp.ev_x0))) return rc;
        (void)hipEventRecord(e->dp.ev_g[cur], e->dp.stream);
    }
    float* gprev = (prv == 1) ? e->dp.grad_alt : e->grad;
    const int apply = e->dp.async_t > 0;
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->dp.ev_g[apply ? prv : cur], 0));     // step 0 only records: it reads its own (reduced) tail
    if ((rc = launch_update(e, update_form(e), apply ? gprev : gcur, apply ? e->dp.dbl_prev : e->sums(), apply ? e->dp.dbl_prev + S_COUNT : e->lsums(),
                            bc_count(e), apply, 0, e->dp.dbl_prev))) return rc;
    e->dp.async_t++;
    return GPE_OK;
}

int gpe_comm_set_async(gpe_engine* e, int on) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->dp.on()) FAIL(e, GPE_ERR_STATE, "gpe_comm_set_async before gpe_comm_init");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipStreamSynchronize(e->dp.stream));
    if (on && !e->dp.grad_alt) {
        HIPCHK(e, hipMalloc((void**)&e->dp.grad_alt, ((size_t)e->P + GT_COUNT) * sizeof(float) + 256));
        HIPCHK(e, hipMalloc((void**)&e->dp.dbl_prev, DBL_COUNT * sizeof(double) + 256));
        HIPCHK(e, hipMemset(e->dp.grad_alt, 0, ((size_t)e->P + GT_COUNT) * sizeof(float)));
        HIPCHK(e, hipMemset(e->dp.dbl_prev, 0, DBL_COUNT * sizeof(double)));
        for (auto& ev : e->dp.ev_g) HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    e->dp.async_grad = on != 0;
    e->dp.async_t = 0;
    return GPE_OK;
}

int gpe_step_dp(gpe_engine* e) {
    if (!e) return GPE_ERR_INVALID;
    if (e->smp.adaptive()) FAIL(e, GPE_ERR_STATE, "gpe_step_dp: the adaptive sampler is single-rank");
    if (!e->dp.on()) FAIL(e, GPE_ERR_STATE, "gpe_step_dp before gpe_comm_init");
    if (e->dp.async()) return step_dp_async(e);
    int rc;
    StepScope seq{e};
    if ((rc = dp_begin(e))) return rc;
    // layer buckets need every map's gradient to be final when its weight kernel ends: no second batch adding to it later
    const bool bucketed = e->path == GPE_PATH_GENERIC && e->cfg.w_sym == 0.f && !e->st.bc_inflight;
    // Fused / wide kernel sets: the next kernel needs each all-reduce's result at once and nothing else is enqueued meanwhile, so the
    // collective goes onto the COMPUTE stream itself -- no event hop to the exchange stream and back (each cross-stream dependency
    // costs several microseconds on this runtime: 4 hops were most of the 35-40 us a world-1 step lost against the plain step,
    // profiles/r04/dp_world1_*.json).  The exchange stream stays for what does overlap: the generic set's layer buckets and the
    // opt-in stale-gradient mode.  GPE_DP_INLINE=0 restores the two-stream form.
    const bool inl = !bucketed && e->dp.inline_sync;
    if ((rc = dp_exchange_sums(e, inl))) return rc;
    if ((rc = step_backward(e, StepOpts{}, bucketed))) return rc;
    // the gradient message: whole, or -- the layers went bucket by bucket -- the exchange tail alone (sum r^2)
    float* msg = bucketed ? e->grad + e->P : e->grad;
    const size_t count = bucketed ? (size_t)GT_COUNT : (size_t)e->P + GT_COUNT;
    if ((rc = dp_allreduce(e, msg, count, ncclFloat, inl ? nullptr : e->dp.ev_x0))) return rc;
    if (!inl && (rc = dp_join(e))) return rc;
    return step_update(e);
}

int gpe_run_dp(gpe_engine* e, int64_t n_steps) {
    if (e && e->smp.adaptive()) FAIL(e, GPE_ERR_STATE, "gpe_run_dp: the adaptive sampler is single-rank");
    for (int64_t i = 0; i < n_steps; ++i) {
        int rc = gpe_step_dp(e);
        if (rc) return rc;
    }
    return GPE_OK;
}

int gpe_exchange_sums(gpe_engine* e, void** p, int64_t* count) {
    if (!e || !p || !count) return GPE_ERR_INVALID;
    *p = e->sums(); *count = S_COUNT;
    return GPE_OK;
}
int gpe_exchange_grad(gpe_engine* e, void** p, int64_t* count) {
    if (!e || !p || !count) return GPE_ERR_INVALID;
    *p = e->grad; *count = e->P + GT_COUNT;
    return GPE_OK;
}

int gpe_read_scalars(gpe_engine* e, gpe_scalars* out) {
    if (!e || !out) return GPE_ERR_INVALID;
    if (int rc = last_record_read(e, out)) return rc;
    if (out->nonfinite != 0.0) FAIL(e, GPE_ERR_NONFINITE, "non-finite loss or gradient at step %lld; parameters not updated", (long long)out->step + 1);
    return GPE_OK;
}

int gpe_read_history(gpe_engine* e, int64_t first, int64_t count, gpe_scalars* out) {
    if (!e || !out || first < 1 || count < 0) return GPE_ERR_INVALID;
    if (count > e->cap) FAIL(e, GPE_ERR_INVALID, "history window larger than capacity %d", e->cap);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int64_t i = 0; i < count;) {
        int64_t slot = (first - 1 + i) % e->cap;
        int64_t run = std::min<int64_t>(count - i, e->cap - slot);
        HIPCHK(e, hipMemcpy(out + i, e->hist + slot, run * sizeof(gpe_scalars), hipMemcpyDeviceToHost));
        i += run;
    }
    return GPE_OK;
}

// One whole step: begin, backward and update enqueued back to back (callers pass head_may_fuse and update_may_fuse: the head may ride
// in the forward kernel, the update in the slab reduction).  A phase that fails clears the per-step record itself.
static int whole_step(gpe_engine* e, StepOpts o) {
    int rc = step_begin(e, o);
    if (!rc) rc = step_backward(e, o);
    if (!rc) rc = step_update(e);
    return rc;
}

int gpe_step(gpe_engine* e, gpe_scalars* out) {
    int rc;
    if (!e) return GPE_ERR_INVALID;
    if ((rc = whole_step(e, StepOpts{/*head_may_fuse=*/true, /*update_may_fuse=*/true}))) return rc;
    if ((rc = monitor_after_steps(e, 1))) return rc;
    if (out) return gpe_read_scalars(e, out);
    return GPE_OK;
}

// Everything a captured step bakes into its kernel nodes: physics and optimiser constants, batch geometry and pointers.  A replay is valid
// while this key is unchanged, so whatever a capture freezes must be in it or follow from something that is.  Checklist for a new field:
//   by-value arguments    Phys and OptCfg whole (every loss weight, gamma, p, n_global / W, n_orth, the mixture couplings), base_norm, the
//                         boundary count handed to the update (follows from bc.n / main.n and pts.na)
//   pointers              per batch the point, potential, output, head and activation buffers listed below; S[], Z0 / Z1, A2 and ld are
//                         allocated by setup_batch together with O, Ob, A0 and A1 and for the same (n, C), so they move only when those do;
//                         gslab, Wpk / WpkT and head_slots are allocated once at gpe_create; bc_target, grad, dbl, wq, orth_host[] (caller
//                         arrays, frozen states, the precomputed base)
//   host-side branches    head in the forward kernel or not and seeds in the reverse kernel or not (n, wq, Phys), boundary rows merged or
//                         forked to the side stream (main.pts.b, bc.n), weighted or unweighted head / seed kernels (wq)
// Device-resident state (parameters, Adam moments, OptDev, the contents of any bound array) is read afresh by every replay and needs no
// entry.  A new setter or bind gets its row in tests/live_table.py, which runs a live capture against it on every kernel family.
static std::vector<char> graph_key_of(gpe_engine* e) {
    std::vector<char> k;
    auto put = [&](const void* p, size_t n) { const char* c = (const char*)p; k.insert(k.end(), c, c + n); };
    put(&e->ph, sizeof e->ph); put(&e->oc, sizeof e->oc); put(&e->base_norm, sizeof e->base_norm);
    for (Batch* b : {&e->main, &e->bc, &e->sym}) {
        const void* ptrs[] = {b->pts.a, b->pts.b, b->V, b->O, b->Ob, b->u, b->Hu, b->ux, b->stored, b->A0, b->A1};
        put(&b->pts.na, sizeof b->pts.na);
        put(ptrs, sizeof ptrs); put(&b->n, sizeof b->n); put(&b->C, sizeof b->C);
    }
    const void* more[] = {e->bc_target, e->grad, e->dbl, e->stream, e->wq};
    put(more, sizeof more); put(e->orth_host, sizeof e->orth_host);
    put(&e->cfg.w_bc, sizeof e->cfg.w_bc); put(&e->cfg.w_sym, sizeof e->cfg.w_sym);
    return k;
}

static void graph_drop(gpe_engine* e) {
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }
    e->graph_key.clear();
}

// capture begin + backward + update on the private capture stream (the caller's stream may be the legacy null stream, which
// cannot be captured); the instantiated graph is launched on the caller's stream.
static int graph_build(gpe_engine* e) {
    graph_drop(e);
    if (!e->cap_stream && hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking) != hipSuccess) return GPE_ERR_HIP;
    std::vector<char> key = graph_key_of(e);
    e->packed_dirty = true;                       // the captured step always starts with k_begin
    e->acc_clean = false;
    hipGraph_t g = nullptr;
    int rc = GPE_OK;
    Redirect to_capture(e, e->cap_stream, e->grad, e->gslab);       // (nothing below enqueues on the caller's stream)
    if (hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return GPE_ERR_HIP;
    // graph_steps consecutive steps per graph: ONE hipGraphLaunch then enqueues all their kernels -- at the reference's batch sizes the
    // host's ~7 us per launch is as long as the kernels themselves (a one-step graph costs more per replay than it saves)
    // (a redraw is never recorded: a replay runs on whatever set the buffer holds)
    for (int sidx = 0; sidx < e->graph_steps && !rc; ++sidx) rc = whole_step(e, StepOpts{/*head_may_fuse=*/true, /*update_may_fuse=*/true, /*capturing=*/true});
    hipError_t st = hipStreamEndCapture(e->cap_stream, &g);
    e->packed_dirty = true;                       // nothing ran during capture
    e->acc_clean = false;
    if (rc || st != hipSuccess || !g) { if (g) (void)hipGraphDestroy(g); (void)hipGetLastError(); return rc ? rc : GPE_ERR_HIP; }
    st = hipGraphInstantiate(&e->graph_exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (st != hipSuccess) { e->graph_exec = nullptr; (void)hipGetLastError(); return GPE_ERR_HIP; }
    e->graph_key.swap(key);
    return GPE_OK;
}

// one replay: graph_steps whole steps in one launch.  The redraw a replay may start with is enqueued here, outside the graph
static int graph_replay(gpe_engine* e) {
    if (e->smp.bound()) {
        int rc = sampler_before_step(e, /*capturing=*/false);
        if (rc) return rc;
        e->smp.steps += e->graph_steps;
    }
    HIPCHK(e, hipGraphLaunch(e->graph_exec, e->stream));
    after_update(e);
    e->st = StepState{};
    return monitor_after_steps(e, e->graph_steps);
}
// true: gpe_run may replay -- the run is eligible and a graph of the engine as it stands exists (built here when the key changed; a build
// that fails falls back to plain launches for good)
static bool graph_ready(gpe_engine* e, int64_t n_steps) {
    if (!(e->use_graph && !e->prof && n_steps >= e->graph_steps && e->main.n > 0 && (e->graph_forced || e->main.n <= e->graph_max_points))) return false;
    if ((!e->graph_exec || e->graph_key != graph_key_of(e)) && graph_build(e) != GPE_OK) { graph_drop(e); e->use_graph = false; }
    return e->graph_exec != nullptr;
}

int gpe_run(gpe_engine* e, int64_t n_steps) {
    if (!e) return GPE_ERR_INVALID;
    const bool graph = graph_ready(e, n_steps);
    for (int64_t done = 0; done < n_steps;) {
        // a replay must not run past a monitor step, nor across a redraw of the sampler: up to there with plain launches when fewer than
        // a graph's steps are left to it
        int64_t room = e->mon.bound() ? e->mon.room() : e->graph_steps;
        if (e->smp.bound()) room = std::min(room, e->smp.every - e->smp.steps % e->smp.every);
        const bool replay = graph && n_steps - done >= e->graph_steps && room >= e->graph_steps;
        const int rc = replay ? graph_replay(e) : gpe_step(e, nullptr);
        if (rc) return rc;
        done += replay ? e->graph_steps : 1;
    }
    return GPE_OK;
}

// the opening of a forward-only detour on the bound set (gpe_residual, gpe_mixture_energy).  It clears the per-step record itself and
// files nothing in it, so the caller's StepScope starts behind it
static int detour_begin(gpe_engine* e, const char* who) {
    if (e->main.n <= 0) FAIL(e, GPE_ERR_STATE, "%s before bind_points", who);
    e->st = StepState{};                          // forward-only evaluation: k_head_pde forms the sums, never the slots of an earlier step
    int rc = launch_begin(e, /*force=*/true);     // no reverse pass here: the gradient buffer must read zero
    return rc ? rc : mlp_forward(e, e->main, false);
}

int gpe_residual(gpe_engine* e, gpe_scalars* out, float* d_psi, float* d_resid) {
    if (!e || !out) return GPE_ERR_INVALID;
    int rc;
    if ((rc = detour_begin(e, "residual"))) return rc;
    StepScope seq{e};
    if ((rc = launch_head_pde(e))) return rc;
    if (e->cfg.w_sym != 0.f) {
        if ((rc = mlp_forward(e, e->sym, false))) return rc;
        if ((rc = launch_head_sym(e))) return rc;
    }
    if ((rc = launch_seed_pde(e, d_resid, 0, /*head_slots=*/0))) return rc;
    if ((rc = bc_fork(e, false))) return rc;
    if ((rc = bc_join(e))) return rc;
    if (d_psi) hipLaunchKernelGGL(k_copy_psi, dim3(cdiv(e->n_pde, 256)), dim3(256), 0, e->stream, e->main.u, d_psi, e->n_pde,
                                  e->main.ld, e->nd.n_out);
    if ((rc = launch_tail(e, false))) return rc;
    if ((rc = launch_update(e, update_form(e), e->grad, e->sums(), e->lsums(), bc_count(e), 0, 0, nullptr))) return rc;
    return last_record_read(e, out);
}

int gpe_set_gamma(gpe_engine* e, float g) { if (!e) return GPE_ERR_INVALID; e->cfg.gamma = g; fill_phys(e); return GPE_OK; }
int gpe_set_mixture(gpe_engine* e, float g11, float g22, float g12) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->cfg.mixture) FAIL(e, GPE_ERR_STATE, "set_mixture: not a mixture engine (gpe_config.mixture)");
    if (!__builtin_isfinite(g11) || !__builtin_isfinite(g22) || !__builtin_isfinite(g12)) FAIL(e, GPE_ERR_INVALID, "set_mixture: couplings must be finite");
    e->cfg.mix_g[0] = g11; e->cfg.mix_g[1] = g22; e->cfg.mix_g[2] = g12; fill_phys(e); return GPE_OK;
}
int gpe_mixture_scalars(gpe_engine* e, double out[8]) {
    if (!e || !out) return GPE_ERR_INVALID;
    if (!e->cfg.mixture) FAIL(e, GPE_ERR_STATE, "mixture_scalars: not a mixture engine (gpe_config.mixture)");
    OptDev h;
    if (int rc = opt_state_read(e, &h)) return rc;
    for (int k = 0; k < 8; ++k) out[k] = h.mix[k];
    return GPE_OK;
}
int gpe_mixture_energy_weight(gpe_engine* e, float w_E) {
    if (!e) return GPE_ERR_INVALID;
    if (!e->cfg.mixture) FAIL(e, GPE_ERR_STATE, "mixture_energy_weight: not a mixture engine (gpe_config.mixture)");
    if (!__builtin_isfinite(w_E) || w_E < 0.f) FAIL(e, GPE_ERR_INVALID, "mixture_energy_weight: the weight must be finite and >= 0");
    e->mix_wE = w_E; fill_phys(e); return GPE_OK;
}
// Forward-only detour on the bound set, like gpe_residual: value and first-derivative jets, the EN head, no seeds; parameters, optimiser
// state and the last record stay.  The step behind it starts by zeroing the sums filed here (acc_clean is false).
int gpe_mixture_energy(gpe_engine* e, double out[8]) {
    if (!e || !out) return GPE_ERR_INVALID;
    if (!e->cfg.mixture) FAIL(e, GPE_ERR_STATE, "mixture_energy: not a mixture engine (gpe_config.mixture)");
    int rc;
    if ((rc = detour_begin(e, "mixture_energy"))) return rc;
    StepScope seq{e};
    if ((rc = launch_head_pde(e, /*energy=*/true))) return rc;
    if (e->dp.on() && (rc = dp_allreduce(e, e->sums(), S_COUNT, ncclDouble, nullptr))) return rc;      // over all ranks: the first phase's exchange
    double s[S_COUNT];
    HIPCHK(e, hipMemcpyAsync(s, e->sums(), sizeof s, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->acc_clean = false;
    const MixEnergy me = mix_energy_of(e->oc.mix.g, e->oc.mix.n, (double)e->ph.dx, s);
    out[0] = me.E; out[1] = s[S_MIX_T1]; out[2] = s[S_MIX_T2]; out[3] = s[S_MIX_Q11]; out[4] = s[S_MIX_Q22]; out[5] = s[S_MIX_Q12];
    out[6] = s[S_DEN]; out[7] = s[S_MIX_DEN2];
    return GPE_OK;
}
int gpe_set_power(gpe_engine* e, int p) {
    if (!e) return GPE_ERR_INVALID;
    if (e->cfg.mixture && p != 3) FAIL(e, GPE_ERR_INVALID, "a mixture needs p=3");
    if (p < 1 || p > 32) FAIL(e, GPE_ERR_INVALID, "power p must be in [1,32]");
    e->cfg.p = p; fill_phys(e); return GPE_OK;
}
int gpe_set_perturb_scale(gpe_engine* e, float s) { if (!e) return GPE_ERR_INVALID; e->cfg.perturb_scale = s; fill_phys(e); return GPE_OK; }
int gpe_set_loss_weights(gpe_engine* e, const float w[6]) {
    if (!e || !w) return GPE_ERR_INVALID;
    if (w[5] != 0.f && e->nd.n_out != 1 && !(e->cfg.complex_psi && e->nd.n_out == 2 && e->cfg.p == 3))
        FAIL(e, GPE_ERR_INVALID, "the Riesz energy term needs real psi (out=1) or complex psi (out=2) with p = 3");
    if (e->cfg.mixture && (w[3] != 0.f || w[4] != 0.f || w[5] != 0.f)) FAIL(e, GPE_ERR_INVALID, "a mixture has no symmetry, orthogonality or Riesz term");
    if (e->wq && w[3] != 0.f) FAIL(e, GPE_ERR_INVALID, "the symmetry batch has no quadrature weights: w_sym stays 0 while weights are bound");
    if ((w[3] != 0.f) != (e->cfg.w_sym != 0.f)) FAIL(e, GPE_ERR_INVALID, "the symmetry term cannot be switched on/off after bind_points");
    e->cfg.w_pde = w[0]; e->cfg.w_bc = w[1]; e->cfg.w_norm = w[2]; e->cfg.w_sym = w[3]; e->cfg.w_orth = w[4]; e->cfg.w_riesz = w[5];
    fill_phys(e);
    return GPE_OK;
}
int gpe_set_n_global(gpe_engine* e, int64_t n) {
    if (!e) return GPE_ERR_INVALID;
    if (e->wq) FAIL(e, GPE_ERR_STATE, "set_n_global: quadrature weights are bound, N of the means is their total W (gpe_bind_weights)");
    e->cfg.n_global = n; fill_phys(e); return GPE_OK;
}
int gpe_set_lr(gpe_engine* e, float lr) {
    if (!e) return GPE_ERR_INVALID;
    OptDev h;
    if (int rc = opt_state_read(e, &h)) return rc;
    h.lr = lr; h.lr0 = lr;
    return opt_state_write(e, h);
}

int gpe_profile_enable(gpe_engine* e, int on) {
    if (!e) return GPE_ERR_INVALID;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->prof = on != 0;
    e->ev_used = 0;
    return GPE_OK;
}
int gpe_profile_read(gpe_engine* e, double out[4]) {
    if (!e || !out) return GPE_ERR_INVALID;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    out[0] = out[1] = out[2] = out[3] = 0.0;
    for (size_t i = 0; i < e->ev_used; ++i) {
        float ms = 0.f;
        HIPCHK(e, hipEventElapsedTime(&ms, e->ev_pool[2 * i], e->ev_pool[2 * i + 1]));
        out[e->ev_kind[i] ? 2 : 0] += ms;
        out[e->ev_kind[i] ? 3 : 1] += 1.0;
    }
    e->ev_used = 0;
    return GPE_OK;
}

int gpe_stop_state(gpe_engine* e, int* stopped, int64_t* stop_step) {
    if (!e) return GPE_ERR_INVALID;
    OptDev h;
    if (int rc = opt_state_read(e, &h)) return rc;
    if (stopped) *stopped = h.stopped;
    if (stop_step) *stop_step = h.stop_step;
    return GPE_OK;
}

// diagnostic builds (-DGPE_STAMP) only: read and clear the per-phase cycle counters of the reverse kernel
int gpe_debug_read_stamps(gpe_engine* e, unsigned long long out[16]) {
    if (!e || !out) return GPE_ERR_INVALID;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), 16 * sizeof(unsigned long long)));
    unsigned long long z[16] = {0};
    HIPCHK(e, hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z));
    return GPE_OK;
}

#ifdef GPE_STAMP
// tuning builds only (not part of include/gpe_hip.h): the per-workgroup phase trace of f_backward_pipe
extern "C" int gpe_debug_read_trace(gpe_engine* e, unsigned long long* out, int n) {
    if (!e || !out || n > 512 * 4 * 32) return GPE_ERR_INVALID;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace), (size_t)n * sizeof(unsigned long long)));
    return GPE_OK;
}
#endif

int gpe_step_cost(const gpe_engine* e, double* flops_per_point, double* hbm_bytes_per_point) {
    if (!e) return GPE_ERR_INVALID;
    // SURVEY 8(d) with the channel count of the training batches, C = d + 2 (value, d first derivatives, Laplacian) instead of
    // 1 + 2d:  F_fwd = 2 d H + C [2 H^2 (L-1) + 2 H out] (+ activations), F_step = 3 F_fwd ; B_mat = 2 C H L 4
    const int d = e->nd.dim, L = e->nd.n_lin - 1, H = e->nd.width[1], no = e->nd.n_out;
    const double C = d + 2;
    double gemm = 2.0 * d * H + C * (2.0 * H * H * (L - 1) + 2.0 * H * no);
    double act = (double)H * L * (6 + 4 * d);
    if (flops_per_point) *flops_per_point = 3.0 * (gemm + act);
    if (hbm_bytes_per_point) *hbm_bytes_per_point = 2.0 * C * H * L * 4.0;
    return GPE_OK;
}

}  // extern "C"
