"""Every GPE_* run-time switch the library reads (getenv in csrc/gpe_engine.hip and csrc/gpe_wide.hip), with the values the switch
matrix (tests/test_gpu_switch_matrix.py) drives, the network classes each applies to, and what the matrix expects of it.
Plain data: no torch, no HIP -- tests/test_switch_table_cpu.py checks it against the sources on any box.

Row fields
  values      non-default settings to test (each a dict of environment variables; combinations where the switch needs another to act)
  applies_to  predicate over a class descriptor (see CLASS_KEYS): the classes where the switch can change anything
  expect      "kernels"  -- at least one applicable class reports an active_kernels string (fwd, bwd or split) other than its default
              "bitwise"  -- loss, gradient and parameters bit-identical to the default engine's for every applicable class
              "order"    -- only the summation order or the launch geometry changes: the oracle tolerances apply
              "elsewhere:<module path with dots>::<test>" -- not drivable in-process; that test covers it against the oracle
              (every row is also held to the fp64 oracle, whatever its expect)
  multi       also run run(8) behind the first step and follow the per-step loss of the oracle's trajectory
  dp          the step goes through a world-1 native communicator (comm_init(0, 1), step_dp)
  note        what the switch selects
"""

# descriptor keys: H (hidden width as run), maps (hidden -> hidden linear maps), res (residual blocks), n_out, dim,
# path ("fused" | "wide" | "generic": the H = 128 1D / 2D classes are "wide" with the cooperative forward), loss ("plain" | "orth" |
# "sym" | "riesz" | "energy"), pad (hidden widths padded to an instantiated one), large (a large-batch stand-in), P (parameters as run)
CLASS_KEYS = ("H", "maps", "res", "n_out", "dim", "path", "loss", "pad", "large", "P")

# f_forward / f_backward_pipe / f_backward_coop families at H <= 64
def _fused64(d): return d["path"] == "fused" and d["H"] <= 64
def _mlp3(d): return _fused64(d) and not d["res"] and d["maps"] <= 3
# f_backward_pipe: one to three maps, two workgroups' exchange buffers in the LDS (not H = 64 in 3D)
def _pipe(d): return _mlp3(d) and not (d["H"] == 64 and d["dim"] == 3)
# head / seed fusion: real psi, no orthogonality / Riesz / symmetry / regulariser terms
def _head(d): return _fused64(d) and d["n_out"] == 1 and d["loss"] == "plain"
def _seeds(d): return _pipe(d) and _head(d) and not d["large"]
def _h128(d): return d["H"] == 128 and d["dim"] <= 2 and d["path"] in ("fused", "wide")
def _wide(d): return d["path"] == "wide"
# deterministic whole steps (one workgroup per tile, per-workgroup slabs): the classes test_update_kernel_forms_are_bit_identical runs
def _bitwise(d): return _pipe(d) and d["n_out"] == 1 and not d["large"] and d["loss"] in ("plain", "sym")
def _generic(d): return d["path"] == "generic"
def _small_p(d): return d["path"] in ("fused", "wide") and d["P"] < 32768 and not d["large"]
# k_head_pde / k_seed_pde: every loss flavour, one class of each set
def _head_kernel(d): return not d["large"] and (_fused64(d) and d["maps"] <= 3 or d["H"] in (128, 512) and d["dim"] <= 2)

SWITCHES = {
    # ---- path and kernel-set selection at gpe_create ------------------------------------------------------------------------------
    "GPE_PAD_WIDTH": dict(values=[{"GPE_PAD_WIDTH": "0"}], applies_to=lambda d: d["pad"], expect="kernels",
                          note="0: hidden widths without a kernel instance run as given (generic set) instead of zero-padded on the fused set"),
    "GPE_RES_FUSED": dict(values=[{"GPE_RES_FUSED": "0"}], applies_to=lambda d: d["res"] and d["path"] == "fused", expect="kernels",
                          note="0: residual-block networks on the generic set instead of f_forward_coop / f_backward_coop <..., RES>"),
    "GPE_WIDE": dict(values=[{"GPE_WIDE": "0"}, {"GPE_WIDE": "1", "GPE_WIDE_MIN_TILES": "0"}], applies_to=_h128, expect="kernels",
                     note="H = 128 in 1D / 2D: 0 cooperative kernels only, 1 the wide set's forward too (default: its per-map reverse from wide_min_tiles)"),
    "GPE_WIDE_MIN_TILES": dict(values=[{"GPE_WIDE_MIN_TILES": "0"}], applies_to=lambda d: _h128(d) and not d["large"], expect="kernels",
                               note="H = 128 1D / 2D: the per-map reverse kernels w_bwd_map from this many tiles on (default 2 048)"),
    "GPE_WIDE_TOP": dict(values=[{"GPE_WIDE_TOP": "0"}], applies_to=lambda d: _wide(d) and (d["dim"] == 3 or d["H"] == 256 or d["large"]),
                         expect="order", note="wide reverse: 0 = the output layer in a launch of its own (w_bwd_out); read at every launch"),
    "GPE_WIDE_FWD_MT": dict(values=[{"GPE_WIDE_FWD_MT": "1"}], applies_to=_h128,
                            expect="elsewhere:tests.test_gpu_parity::test_multi_tile_wide_forward_kernel_matches_oracle",
                            note="w_forward_mt (several point tiles per pass); read once per process, so run in a child process there"),
    "GPE_COOP": dict(values=[{"GPE_COOP": "0"}, {"GPE_COOP": "0", "GPE_RACC": "0"}, {"GPE_COOP": "-1"},
                             {"GPE_COOP": "2", "GPE_COOP_MAX_TILES": "64"}],
                     applies_to=lambda d: _fused64(d) or _h128(d), expect="kernels",
                     note="cooperative kernels: 0 never (residual blocks keep theirs), 1 always, other values up to GPE_COOP_MAX_TILES tiles"),
    "GPE_COOP_MAX_TILES": dict(values=[{"GPE_COOP": "-1", "GPE_COOP_MAX_TILES": "64"}, {"GPE_COOP": "2", "GPE_COOP_MAX_TILES": "1"}],
                               applies_to=_fused64, expect="kernels",
                               note="GPE_COOP other than 0 / 1: the cooperative reverse kernel for batches up to this many tiles"),
    "GPE_COOP128": dict(values=[{"GPE_COOP128": "0", "GPE_WIDE": "0"}], applies_to=_h128, expect="kernels",
                        note="0: H = 128 leaves the cooperative kernels (f_forward<128> + f_backward<128> on global-atomic slabs)"),
    "GPE_COOP_FWD128": dict(values=[{"GPE_COOP_FWD128": "0"}], applies_to=_h128, expect="kernels",
                            note="0: H = 128 forward on the per-wave-tile f_forward<128> instead of f_forward_coop<128>"),
    "GPE_COOP_FWD_MAX_TILES": dict(values=[{"GPE_COOP_FWD_MAX_TILES": "0"}, {"GPE_COOP_FWD_MAX_TILES": "0", "GPE_FUSE_HEAD_TILE_MIN": "0"}],
                                   applies_to=_mlp3, expect="kernels",
                                   note="H <= 64, one to three maps: the cooperative forward kernel up to this many tiles (default 8 per CU)"),
    "GPE_STAGE_MIN_TILES": dict(values=[{"GPE_COOP": "0", "GPE_STAGE_MIN_TILES": "1000000000"}], applies_to=_mlp3, expect="kernels",
                                note="batches with fewer tiles take the unstaged per-wave-tile kernels (weights from L2, LDS-atomic gradients)"),
    "GPE_RACC": dict(values=[{"GPE_COOP": "0", "GPE_RACC": "0"}], applies_to=_mlp3, expect="kernels",
                     note="0: the per-wave-tile reverse kernel without register-resident weight gradients"),
    "GPE_WLDS": dict(values=[{"GPE_WLDS": "0", "GPE_COOP_FWD_MAX_TILES": "0"}], applies_to=_mlp3, expect="kernels",
                     note="0: f_forward reads the hidden weights from L2 instead of staging them in LDS"),
    "GPE_PIPE": dict(values=[{"GPE_PIPE": "0"}], applies_to=_pipe, expect="kernels",
                     note="0: the two-barrier f_backward_coop instead of the one-barrier-per-map f_backward_pipe"),
    "GPE_FWD_B6": dict(values=[{"GPE_FWD_B6": "1", "GPE_COOP_FWD_MAX_TILES": "0"}, {"GPE_COOP": "0", "GPE_FWD_B6": "1"}],
                       applies_to=_fused64, expect="kernels",
                       note="1: f_forward_b6 (H x H maps as six bf16 products per fp32 product) for the per-wave-tile forward pass"),
    "GPE_BWD_B6": dict(values=[{"GPE_BWD_B6": "1"}, {"GPE_BWD_B6": "1", "GPE_FWD_B6": "1", "GPE_COOP_FWD_MAX_TILES": "0"}],
                       applies_to=_fused64, expect="kernels",
                       note="1: f_backward_coop<..., B6> for plain MLPs of one to three maps (others keep the fp32 kernels)"),
    "GPE_COOP_WG_PER_CU": dict(values=[{"GPE_COOP_WG_PER_CU": "1"}], applies_to=_fused64, expect="order",
                               note="cooperative reverse kernels at H <= 64: persistent workgroups per CU (1..2)"),
    "GPE_FWD_WG_PER_CU": dict(values=[{"GPE_FWD_WG_PER_CU": "1", "GPE_COOP_FWD_MAX_TILES": "0"}], applies_to=_mlp3, expect="order",
                              note="per-wave-tile forward: workgroups per CU (1..GPE_FWD_WAVES; gpe_create refuses more)"),
    # ---- head / seed fusion and tile shares ---------------------------------------------------------------------------------------
    "GPE_FUSE_SEED": dict(values=[{"GPE_FUSE_SEED": "0"}], applies_to=_seeds, expect="kernels",
                          note="0: k_seed_pde forms the seeds instead of the pipelined reverse kernel"),
    "GPE_FUSE_SEED_MAX": dict(values=[{"GPE_FUSE_SEED_MAX": "0"}], applies_to=_seeds, expect="kernels",
                              note="the pipelined reverse kernel forms the seeds up to this many points (default 65 536)"),
    "GPE_FUSE_HEAD": dict(values=[{"GPE_FUSE_HEAD": "0"}], applies_to=_head, expect="kernels",
                          note="0: k_head_pde instead of the head inside the forward kernel"),
    "GPE_FUSE_HEAD_MAX": dict(values=[{"GPE_FUSE_HEAD_MAX": "0"}], applies_to=lambda d: _head(d) and not d["large"], expect="kernels",
                              note="the cooperative forward kernel runs the head up to this many points (default 6 144)"),
    "GPE_FUSE_HEAD_TILE_MIN": dict(values=[{"GPE_COOP_FWD_MAX_TILES": "0", "GPE_FUSE_HEAD_TILE_MIN": "0"},
                                           {"GPE_COOP_FWD_MAX_TILES": "0", "GPE_FUSE_HEAD_TILE_MIN": "1000000000"}],
                                   applies_to=lambda d: _head(d) and d["maps"] <= 3 and not d["res"], expect="kernels",
                                   note="f_forward (per-wave tiles) runs the head from this many points on (default 32 769)"),
    "GPE_SHARE_MIN_TILES": dict(values=[{"GPE_SHARE_MIN_TILES": "1000000"}], applies_to=lambda d: _pipe(d) and d["large"], expect="kernels",
                                note="uneven tile split of two workgroups per CU from this many tiles per workgroup (default 16)"),
    "GPE_PIPE_SHARE": dict(values=[{"GPE_PIPE_SHARE": "0"}, {"GPE_PIPE_SHARE": "700"}], applies_to=lambda d: _pipe(d) and d["large"],
                           expect="kernels", note="f_backward_pipe: share (/1024) of a CU's tiles for its first workgroup; 0 = even"),
    "GPE_FWD_SHARE": dict(values=[{"GPE_FWD_SHARE": "0"}, {"GPE_FWD_SHARE": "300"}], applies_to=lambda d: _mlp3(d) and d["large"],
                          expect="kernels", note="f_forward: the same for its two workgroups per CU; 0 = even"),
    "GPE_HEAD_WG_PER_CU": dict(values=[{"GPE_HEAD_WG_PER_CU": "2", "GPE_FUSE_HEAD": "0"}], applies_to=_head_kernel, expect="order",
                               note="k_head_pde / k_seed_pde: workgroups per CU (bounds the grid at large batches)"),
    "GPE_HEAD_THREADS": dict(values=[{"GPE_HEAD_THREADS": "256", "GPE_FUSE_HEAD": "0"}, {"GPE_HEAD_THREADS": "512"}], applies_to=_head_kernel,
                             expect="order", note="k_head_pde / k_seed_pde: threads per workgroup (256, 512 or 1024)"),
    # ---- generic layer-wise set ---------------------------------------------------------------------------------------------------
    "GPE_GEN_MFMA": dict(values=[{"GPE_GEN_MFMA": "0"}], applies_to=_generic, expect="kernels",
                         note="0: generic set without matrix-core kernels (VALU g_fwd_layer / g_bwd_weight only)"),
    "GPE_GEN_MFMA2": dict(values=[{"GPE_GEN_MFMA2": "0"}], applies_to=_generic, expect="kernels",
                          note="0: no 128 x 128-tile kernels (g_fwd_layer_mfma2 / g_bwd_weight_mfma2) for widths that are multiples of 256 / 128"),
    "GPE_GEN_MIN_CHUNK": dict(values=[{"GPE_GEN_MIN_CHUNK": "256"}, {"GPE_GEN_MIN_CHUNK": "16"}], applies_to=_generic, expect="order",
                              note="g_bwd_weight_mfma: smallest split-K chunk of points (default 32)"),
    # ---- update kernel forms ------------------------------------------------------------------------------------------------------
    "GPE_UPDATE_CACHE": dict(values=[{"GPE_UPDATE_CACHE": "0"}], applies_to=_bitwise, expect="bitwise", multi=True,
                             note="0: the two-pass single-workgroup update (same arithmetic and order: bit for bit, "
                                  "test_update_kernel_forms_are_bit_identical)"),
    "GPE_FUSE_UPDATE": dict(values=[{"GPE_FUSE_UPDATE": "1"}], applies_to=_bitwise, expect="bitwise", multi=True,
                            note="1: the update inside the slab-reduction launch (k_reduce_update; same operations and order)"),
    "GPE_SPLIT_UPDATE": dict(values=[{"GPE_SPLIT_UPDATE": "1"}], applies_to=_small_p, expect="order", multi=True,
                             note="1: slab reduction in the update's partition + the update on 64 workgroups (|g|^2 in another order)"),
    "GPE_UPDATE_MULTI": dict(values=[{"GPE_UPDATE_MULTI": "0"}], applies_to=lambda d: d["P"] >= 32768 and not d["large"], expect="order",
                             multi=True, note="0: the single-workgroup update at every size (default: UPD_G workgroups from 32 768 parameters)"),
    "GPE_UPDATE_MULTI_MIN": dict(values=[{"GPE_UPDATE_MULTI_MIN": "1"}], applies_to=_small_p, expect="order", multi=True,
                                 note="the multi-workgroup update from this many parameters on (|g|^2 summed in another order)"),
    # ---- execution modes ----------------------------------------------------------------------------------------------------------
    "GPE_GRAPH": dict(values=[{"GPE_GRAPH": "0"}, {"GPE_GRAPH": "1"}], applies_to=_bitwise, expect="bitwise", multi=True,
                      note="gpe_run: 0 enqueues every step, 1 replays captured graphs at every size (default: up to 16 384 points)"),
    "GPE_GRAPH_STEPS": dict(values=[{"GPE_GRAPH_STEPS": "1"}, {"GPE_GRAPH_STEPS": "3"}], applies_to=_bitwise, expect="bitwise", multi=True,
                            note="steps captured per graph (default 8); the same kernels in the same order, only fewer per graph launch"),
    "GPE_SIDE_STREAM": dict(values=[{"GPE_SIDE_STREAM": "0"}], applies_to=_bitwise, expect="bitwise", multi=True,
                            note="0: a separate boundary batch runs in line, not on the side stream (the merged default batch: no change)"),
    "GPE_MERGE_BC": dict(values=[{"GPE_MERGE_BC": "0"}, {"GPE_MERGE_BC": "0", "GPE_SIDE_STREAM": "0"}],
                         applies_to=lambda d: _fused64(d) and not d["large"], expect="order", multi=True,
                         note="0: the boundary batch in launches of its own instead of appended to the collocation batch"),
    "GPE_DP_INLINE": dict(values=[{"GPE_DP_INLINE": "0"}], applies_to=lambda d: d["path"] in ("fused", "wide") and not d["large"]
                          and d["loss"] == "plain" and d["maps"] <= 4 and d["n_out"] == 1 and not d["res"] and not d["pad"],
                          expect="order", dp=True,
                          note="0: the data-parallel collectives of a synchronous step on the exchange stream instead of the compute stream"),
}

EXPECTS = ("kernels", "bitwise", "order")
