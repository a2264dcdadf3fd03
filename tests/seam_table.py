"""Every batch size at which the default step (no GPE_* switch set) changes what or how it launches: the thresholds of
csrc/gpe_engine.hip, as functions of the CU count.  tests/test_seam_table_cpu.py holds the defaults named here to the source;
tests/test_gpu_seams.py finds the visible seams again by bisection of active_kernels and runs both sides of every seam against the
fp64 oracle.  Plain data: no torch, no HIP.

A seam is written lower | upper: the last size of the lower regime and the first of the upper one (upper = lower + 1).

What a threshold counts.  Most conditions read main.n, the LAUNCHED batch: the bound collocation points plus the boundary points
merged behind them (nb points ride along when 8 nb <= N, GPE_MERGE_BC).  With the five boundary points of the seam cells the
collocation count at such a seam is five lower than the launched one: 6 139 | 6 140 bound points launch 6 144 | 6 145.  The upper side's
last tile then holds one point, and that point is a boundary point.  fuse_seed_max and the seed kernel's grid count the collocation
points alone (n_pde).  Row field `counts` says which; bound_n() converts.

Row fields
  origin      the struct member / macro of gpe_engine.hip the seam comes from (DEFAULTS gives the value the formula assumes)
  lower       cu -> last size of the lower regime, in the unit of `counts`; None: a device with that many CUs has no such seam
  counts      "launch" (main.n) | "pde" (n_pde) | "obs" (the points handed to observables() / the monitor: not a step at all)
  applies_to  predicate over a class descriptor (keys of tests/switch_table.py, without "large" and "pad")
  visible     active_kernels differs across the seam
  below/above {active_kernels key: regular expression} the string must match on that side (visible rows)
  cells       the classes of tests/test_gpu_seams.py that run this seam against the oracle
  note        what changes
"""
import re

# defaults of the sources the formulas below are written for: name -> (regular expression over the source, value[, file of csrc/ if not
# gpe_engine.hip]).
# tests/test_seam_table_cpu.py fails when one of them moves or disappears.
DEFAULTS = {
    "fuse_head_max": (r"int64_t\s+fuse_head_max\s*=\s*(\d+)\s*;", 6144),
    "fuse_head_tile_min": (r"int64_t\s+fuse_head_tile_min\s*=\s*(\d+)\s*;", 32769),
    "fuse_seed_max": (r"int64_t\s+fuse_seed_max\s*=\s*(\d+)\s*;", 65536),
    "share_min_tiles": (r"int\s+share_min_tiles\s*=\s*(\d+)\s*;", 16),
    "fwd_share": (r"int\s+fwd_share\s*=\s*(\d+)\s*;", 640),
    "pipe_share": (r"int\s+pipe_share\s*=\s*(\d+)\s*;", 576),
    "wide_min_tiles": (r"int64_t\s+wide_min_tiles\s*=\s*(\d+)\s*;", 2048),
    "graph_max_points": (r"int64_t\s+graph_max_points\s*=\s*(\d+)\s*;", 16384),
    "coop_wg_per_cu": (r"int\s+coop_wg_per_cu\s*=\s*(\d+)\s*;", 2),
    "fwd_wg_per_cu": (r"int\s+fwd_wg_per_cu\s*=\s*(\d+)\s*;", 2),
    "head_wg_per_cu": (r"int\s+head_wg_per_cu\s*=\s*(\d+)\s*;", 1),
    "head_threads": (r"int\s+head_threads\s*=\s*(\d+)\s*;", 1024),
    "coop_fwd_tiles_per_cu": (r"coop_fwd_max_tiles\s*=\s*env_i64\(\s*\"GPE_COOP_FWD_MAX_TILES\"\s*,\s*\(int64_t\)e->num_cu\s*\*\s*(\d+)\s*\)\s*;", 8),
    "HEAD_SLOTS": (r"#define\s+HEAD_SLOTS\s+(\d+)", 512),
    "merge_bc_ratio": (r"e->nb_user\s*\*\s*(\d+)\s*<=\s*e->n_pde", 8),
    "gen_min_chunk": (r"int64_t\s+gen_min_chunk\s*=\s*(\d+)\s*;", 32),
    "gen_mfma2_min_chunk": (r"if\s*\(chunk\s*<\s*(\d+)\)\s*chunk\s*=\s*\1\s*;", 256),
    "gen_mfma2_blocks_per_cu": (r"want\s*=\s*\(int64_t\)e->num_cu\s*\*\s*(\d+)\s*/\s*\(\(Ho\s*/\s*128\)", 4),
    "gen_mfma_waves_per_cu": (r"want\s*=\s*\(int64_t\)e->num_cu\s*\*\s*(\d+)\s*/\s*\(\(Ho\s*/\s*64\)", 16),
    "OBS_THREADS": (r"#define\s+OBS_THREADS\s+(\d+)", 256, "gpe_observe.h"),
    "OBS_MAX_WG": (r"#define\s+OBS_MAX_WG\s+(\d+)", 1024, "gpe_observe.h"),
    "wide_group_multiple": (r"if\s*\(g\s*>=\s*(\d+)\)\s*g\s*&=\s*~\(int64_t\)7;", 8, "gpe_wide.hip"),
}
D = {k: v[1] for k, v in DEFAULTS.items()}
TILE = 16          # points per tile (F_TILE)


# ---- class predicates (descriptor keys: H, maps, res, n_out, dim, path, loss) ---------------------------------------------------------
def _fused64(d): return d["path"] == "fused" and d["H"] <= 64
def _mlp3(d): return _fused64(d) and not d["res"] and d["maps"] <= 3
def _pipe(d): return _mlp3(d) and not (d["H"] == 64 and d["dim"] == 3)
def _head(d): return _fused64(d) and d["n_out"] == 1 and d["loss"] == "plain"
def _h128(d): return d["path"] != "generic" and d["H"] == 128 and d["dim"] <= 2
# head_fusable_coop: the reverse pass must form the seeds (pipelined kernel) or the network be deep / residual (k_seed_pde adds the triples)
def _head_coop(d): return _head(d) and (_pipe(d) or d["res"] or d["maps"] > 3)
# the wide set's own forward (w_forward): H = 256, H = 128 in 3D
def _wide_fwd(d): return d["path"] == "wide" and (d["H"] == 256 or d["dim"] == 3)
def _gen_mfma2(d): return d["path"] == "generic" and d["H"] % 128 == 0
def _gen_mfma(d): return d["path"] == "generic" and d["H"] % 64 == 0 and d["H"] % 128 != 0


def _coop_fwd_last(cu): return TILE * D["coop_fwd_tiles_per_cu"] * cu


def _head_tile_last(cu):
    """head_fusable_tile: f_forward must run (past coop_fwd_max_tiles), from fuse_head_tile_min points on, and its grid -- at its cap
    fwd_wg_per_cu * cu from there on -- must fit HEAD_SLOTS: beyond 256 CUs it does not, and the head never moves into f_forward"""
    if D["fwd_wg_per_cu"] * cu > D["HEAD_SLOTS"]:
        return None
    return max(D["fuse_head_tile_min"] - 1, _coop_fwd_last(cu))


SEAMS = {
    "bc_merge": dict(
        origin="merge_bc_ratio", lower=lambda cu: D["merge_bc_ratio"] * NB - 1, counts="pde", visible=False, applies_to=lambda d: True,
        cells=("A", "B"),
        note="the boundary points run as a batch of their own (side stream) | ride behind the collocation points in the same launches"),
    "wide_groups_round": dict(
        origin="wide_group_multiple", lower=lambda cu: TILE * D["wide_group_multiple"], counts="launch", visible=False, applies_to=_wide_fwd,
        cells=("w256",),
        note="w_bwd_map: the workgroup count is rounded down to a multiple of 8 from 8 tiles on, so a workgroup takes a second tile"),
    "gen_mfma_second_block": dict(
        origin="gen_min_chunk", lower=lambda cu: 4 * D["gen_min_chunk"], counts="launch", visible=False, applies_to=_gen_mfma, cells=("gres",),
        note="g_bwd_weight_mfma: a wave per split-K chunk of gen_min_chunk points, four to a workgroup: the grid grows to two"),
    "gen_mfma2_second_chunk": dict(
        origin="gen_mfma2_min_chunk", lower=lambda cu: D["gen_mfma2_min_chunk"], counts="launch", visible=False, applies_to=_gen_mfma2,
        cells=("g512",), note="g_bwd_weight_mfma2: one split-K chunk of 256 points | two, the second with a single point"),
    "head_one_workgroup": dict(
        origin="head_threads", lower=lambda cu: D["head_threads"], counts="launch", visible=False,
        applies_to=lambda d: _fused64(d) and not _head(d), cells=("cplx",),
        note="k_head_pde goes from one workgroup (sums bit-reproducible) to two, each ending in a double atomic; classes whose head "
             "no forward kernel runs"),
    "wide256_groups_cap": dict(
        origin="wide_groups", lower=lambda cu: TILE * (cu // 2 // 8 * 8), counts="launch", visible=False,
        applies_to=lambda d: d["path"] == "wide" and d["H"] == 256, cells=("w256",),
        note="w_bwd_map at H = 256 (two workgroups per tile group): cu / 2 groups reached, groups loop over tiles (H = 128 in 3D: cu groups, "
             "at wide_fwd_grid_cap)"),
    "wide_fwd_grid_cap": dict(
        origin="launch_fwd", lower=lambda cu: TILE * cu, counts="launch", visible=False, applies_to=_wide_fwd, cells=("w256",),
        note="w_forward (one 8-wave workgroup per tile) reaches its grid cap of one workgroup per CU"),
    "coop128_grid_cap": dict(
        origin="fused_grid(n, 1, 1)", lower=lambda cu: TILE * cu, counts="launch", visible=False, applies_to=_h128, cells=("w128",),
        note="f_forward_coop<128> / f_backward_coop<128> (one 8-wave workgroup per CU) reach their grid cap: workgroups loop over tiles"),
    "fuse_head_max": dict(
        origin="fuse_head_max", lower=lambda cu: D["fuse_head_max"] if D["fuse_head_max"] <= _coop_fwd_last(cu) else None, counts="launch",
        visible=True, applies_to=_head_coop,
        below={"fwd": r"^f_forward_coop<[\d,]+,head>$"}, above={"fwd": r"^(?!f_forward_coop<.*,head>$)f_forward"},
        cells=("A", "B", "NS", "deep", "res"),
        note="the head leaves f_forward_coop: k_head_pde runs (and k_seed_pde adds nothing from head_slots)"),
    "coop_grid_cap": dict(
        origin="fused_grid(n, 1, coop_wg_per_cu)", lower=lambda cu: TILE * D["coop_wg_per_cu"] * cu, counts="launch", visible=False,
        applies_to=_fused64, cells=("A", "B", "NS", "deep", "res", "cplx"),
        note="every cooperative kernel at H <= 64 (a workgroup per tile, two per CU) reaches its grid cap: workgroups loop over tiles"),
    "graph_max_points": dict(
        origin="graph_max_points", lower=lambda cu: D["graph_max_points"], counts="launch", visible=False, applies_to=lambda d: True,
        cells=("A", "B", "NS"),
        note="gpe_run replays captured graphs | enqueues every step"),
    "wide_min_tiles": dict(
        origin="wide_min_tiles", lower=lambda cu: TILE * (D["wide_min_tiles"] - 1), counts="launch", visible=True, applies_to=_h128,
        below={"bwd": r"^f_backward_coop<128,"}, above={"bwd": r"w_bwd_map<128,"}, cells=("w128",),
        note="H = 128 in 1D / 2D: single cooperative reverse launch | one w_bwd_map launch per map"),
    "coop_fwd_max_tiles": dict(
        origin="coop_fwd_max_tiles", lower=_coop_fwd_last, counts="launch", visible=True, applies_to=_mlp3,
        below={"fwd": r"^f_forward_coop<"}, above={"fwd": r"^f_forward<"}, cells=("A", "B", "NS"),
        note="f_forward_coop | per-wave-tile f_forward, whose grid fused_grid(n, 4, fwd_wg_per_cu) is at its cap from the same size on "
             "(both are 8 tiles per CU)"),
    "fuse_head_tile_min": dict(
        origin="fuse_head_tile_min", lower=_head_tile_last, counts="launch", visible=True,
        applies_to=lambda d: _head(d) and _mlp3(d), below={"fwd": r"^(f_forward_coop<.*>|f_forward<[\w,]+(?<!,head)>)$"},
        above={"fwd": r"^f_forward<[\w,]+,head>$"}, cells=("A", "B", "NS"),
        note="the head moves into f_forward (needs the per-wave-tile kernel: the later of the two thresholds; the same size at 256 CUs; "
             "no such seam where the capped grid exceeds HEAD_SLOTS)"),
    "gen_mfma2_chunk_grows": dict(
        origin="gen_mfma2_blocks_per_cu", lower=lambda cu: D["gen_mfma2_min_chunk"] * (cu * D["gen_mfma2_blocks_per_cu"] // 16 + 1), counts="launch",
        visible=False, applies_to=lambda d: _gen_mfma2(d) and d["H"] == 512, cells=("g512",),
        note="g_bwd_weight_mfma2 at 512 x 512 (16 block tiles): the chunk count reaches 4 cu / 16 + 1 and the chunks grow past 256 points"),
    "fuse_seed_max": dict(
        origin="fuse_seed_max", lower=lambda cu: D["fuse_seed_max"], counts="pde", visible=True, applies_to=lambda d: _pipe(d) and _head(d),
        below={"bwd": r"^f_backward_pipe<[\d,]+,seeds>$"}, above={"bwd": r"^f_backward_pipe<[\d,]+>$"}, cells=("A", "B"),
        note="f_backward_pipe<..., seeds> | k_seed_pde + f_backward_pipe"),
    "pipe_share": dict(
        origin="share_min_tiles", lower=lambda cu: TILE * (D["share_min_tiles"] * D["coop_wg_per_cu"] * cu - 1), counts="launch", visible=True,
        applies_to=_pipe, below={"split": r"bwd 0/1024$"}, above={"split": rf"bwd {D['pipe_share']}/1024$"}, cells=("A",),
        note="f_backward_pipe: uneven split of a CU's tiles between its two workgroups from share_min_tiles tiles per workgroup on"),
    "gen_mfma_chunk_grows": dict(
        origin="gen_mfma_waves_per_cu", lower=lambda cu: D["gen_min_chunk"] * (cu * D["gen_mfma_waves_per_cu"] + 1), counts="launch", visible=False,
        applies_to=lambda d: _gen_mfma(d) and d["H"] == 64, cells=("gres",),
        note="g_bwd_weight_mfma at 64 x 64: the chunk count reaches 16 cu + 1 and the chunks grow past gen_min_chunk points"),
    "obs_grid_cap": dict(
        origin="OBS_MAX_WG", lower=lambda cu: D["OBS_THREADS"] * D["OBS_MAX_WG"], counts="obs", visible=False, applies_to=lambda d: True, cells=("A",),
        note="k_obs_pass1 / k_obs_pass2 (observables, monitor): one point per thread | the grid at its cap, threads loop over points"),
    "head_grid_cap": dict(
        origin="head_grid(main.n)", lower=lambda cu: D["head_threads"] * D["head_wg_per_cu"] * cu, counts="launch", visible=False,
        applies_to=lambda d: not (_head(d) and _mlp3(d)), cells=("cplx",),
        note="k_head_pde (one point per thread) reaches its grid cap; the classes whose head no forward kernel runs at this size"),
    "seed_grid_cap": dict(
        origin="head_grid(n_pde)", lower=lambda cu: D["head_threads"] * D["head_wg_per_cu"] * cu, counts="pde", visible=False,
        applies_to=lambda d: True, cells=("A",),
        note="k_seed_pde (one point per thread, head_wg_per_cu workgroups per CU) reaches its grid cap: threads loop over points"),
    "fwd_share": dict(
        origin="share_min_tiles", lower=lambda cu: TILE * (4 * D["share_min_tiles"] * D["fwd_wg_per_cu"] * cu - 1), counts="launch",
        visible=True, applies_to=_mlp3, below={"split": r"^fwd 0/1024"}, above={"split": rf"^fwd {D['fwd_share']}/1024"}, cells=("A",),
        note="f_forward: the same split from share_min_tiles tiles per wave on"),
}

# ---- the classes of the seam cells: the smallest network of each kernel family -------------------------------------------------------
# name: (oracle Problem keywords (net_kind as a number: 0 MLP, 1 residual blocks), descriptor)
NB = 5              # boundary points of every class
CLASSES = {
    "A": (dict(layers=[2, 32, 32, 1], gamma=10.0, dx=0.01),
          dict(H=32, maps=1, res=False, n_out=1, dim=2, path="fused", loss="plain")),
    "B": (dict(layers=[1, 64, 64, 64, 1], activation=1, gamma=5.0, base_mode=0, perturb_scale=0.05, dx=0.01),
          dict(H=64, maps=2, res=False, n_out=1, dim=1, path="fused", loss="plain")),
    "NS": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=500.0, dx=0.001),
           dict(H=64, maps=3, res=False, n_out=1, dim=2, path="fused", loss="plain")),
    "deep": (dict(layers=[2, 32, 32, 32, 32, 32, 1], gamma=10.0, dx=0.01),
             dict(H=32, maps=4, res=False, n_out=1, dim=2, path="fused", loss="plain")),
    "res": (dict(layers=[1, 64, 64, 1], net_kind=1, activation=1, kinetic_coeff=1.0, gamma=2.0, base_mode=0, perturb_scale=0.05, dx=0.01),
            dict(H=64, maps=2, res=True, n_out=1, dim=1, path="fused", loss="plain")),
    "cplx": (dict(layers=[2, 64, 64, 2], complex_psi=True, gamma=30.0, omega_rot=0.8, dx=0.01),
             dict(H=64, maps=1, res=False, n_out=2, dim=2, path="fused", loss="plain")),
    "w128": (dict(layers=[2, 128, 128, 1], gamma=10.0, dx=0.001),
             dict(H=128, maps=1, res=False, n_out=1, dim=2, path="wide", loss="plain")),
    # the wide set alone (w_forward, w_bwd_map), and the generic set's two split-K weight-gradient kernels
    "w256": (dict(layers=[3, 256, 256, 256, 1], gamma=100.0, omega=(1.0, 1.4, 2.0), dx=0.01),
             dict(H=256, maps=2, res=False, n_out=1, dim=3, path="wide", loss="plain")),
    "g512": (dict(layers=[2, 512, 512, 1], gamma=10.0, dx=0.01),
             dict(H=512, maps=1, res=False, n_out=1, dim=2, path="generic", loss="plain")),
    "gres": (dict(layers=[1, 64, 64, 64, 64, 1], net_kind=1, activation=1, kinetic_coeff=1.0, gamma=3.0, base_mode=1, perturb_scale=0.05, dx=0.01),
             dict(H=64, maps=6, res=True, n_out=1, dim=1, path="generic", loss="plain")),
}


def bound_n(row, cu, nb=NB):
    """collocation points to bind so that the batch sits on the LOWER side of the seam (the upper side: one more)"""
    n = row["lower"](cu)
    if n is None or row["counts"] != "launch":
        return n
    return n - nb if n - nb >= D["merge_bc_ratio"] * nb else n          # (too few points to merge: launched = bound)


def class_seams(cls, cu, nb=NB):
    """[(bound collocation count of the lower side, [row names])] of the class, ascending; rows that land on one size are one seam"""
    d = CLASSES[cls][1]
    at = {}
    for name, row in SEAMS.items():
        if row["applies_to"](d) and row["counts"] != "obs" and bound_n(row, cu, nb) is not None:
            at.setdefault(bound_n(row, cu, nb), []).append(name)
    return sorted(at.items())


def cells(cu, nb=NB):
    """[(class, bound count of the lower side, [row names])]: what tests/test_gpu_seams.py runs against the oracle"""
    out = []
    for cls in CLASSES:
        for n, names in class_seams(cls, cu, nb):
            if any(cls in SEAMS[r]["cells"] for r in names):
                out.append((cls, n, names))
    return out


def expected(cls, n_bound, cu, nb=NB):
    """{active_kernels key: [regular expressions]} the class's strings must match with n_bound collocation points bound"""
    d = CLASSES[cls][1]
    exp = {}
    for name, row in SEAMS.items():
        if row["visible"] and row["applies_to"](d) and bound_n(row, cu, nb) is not None:
            side = "below" if n_bound <= bound_n(row, cu, nb) else "above"
            for k, rx in row[side].items():
                exp.setdefault(k, []).append(rx)
    return exp


def mismatches(kern, exp):
    return [f"{k}={kern.get(k)!r} does not match {rx!r}" for k, rxs in exp.items() for rx in rxs if not re.search(rx, kern.get(k, ""))]


def inputs(cls, n, seed=0):
    """points, parameters and boundary points of a seam cell (the recipe of tests/test_gpu_parity._inputs / _scale; five boundary
    points in 1D too), numpy float32"""
    import numpy as np
    from oracle import gpe_oracle as go
    kw = CLASSES[cls][0]
    layers = kw["layers"]
    d = layers[0]
    rng = np.random.default_rng(seed)
    x = (np.linspace(-6, 6, n).reshape(-1, 1) if d == 1 else rng.uniform(-3, 3, (n, d))).astype(np.float32)
    w = max(layers[1:-1])
    scale = 0.3 if w <= 64 else (0.15 if w <= 128 else (0.1 if w <= 256 else 0.06))
    flat = (rng.normal(0, 1, go.param_count(layers, kw.get("net_kind", 0))) * scale).astype(np.float32)
    x_bc = (np.array([[-6.0], [6.0], [-6.0], [6.0], [-6.0]]) if d == 1 else rng.uniform(-3, 3, (NB, d))).astype(np.float32)
    return x, flat, x_bc
