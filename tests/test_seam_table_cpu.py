"""The seam table (tests/seam_table.py) against csrc/gpe_engine.hip: every default the table's formulas use is parsed out of the
source, so a retuned threshold fails here until the table moves with it.  And the bound the GPU tests put on the gradient per
parameter block (5e-5 of the block's maximum) is one fp32 can meet: the oracle run in float32 against itself in float64 stays below
1e-5 per block on every seam cell and on every cell of the two older tables the bound was added to."""
import os
import re

import numpy as np
import pytest

from oracle import gpe_oracle as go
from tests import helpers as H
from tests import seam_ref as R
from tests import seam_table as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gross-pitaevskii-eigenvalue-problem_amd", "csrc")
FP32_BLOCK = 1e-5


def source(unit="gpe_engine.hip"):
    with open(os.path.join(CSRC, unit)) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(S.DEFAULTS))
def test_the_default_the_table_assumes_is_the_one_in_the_source(name):
    rx, value, unit = (S.DEFAULTS[name] + ("gpe_engine.hip",))[:3]
    found = re.findall(rx, source(unit))
    assert len(found) == 1, f"{name}: {len(found)} matches of {rx!r} in {unit} -- the default moved or disappeared"
    assert int(found[0]) == value, f"{name} is {found[0]} in {unit}, {value} in tests/seam_table.py: move the table's rows with it"


def test_the_conditions_compare_the_way_the_table_says():
    """inclusive / exclusive ends and the count each condition reads, as literal source text"""
    src = source()
    for text in ("e->main.n <= e->fuse_head_max", "e->main.n >= e->fuse_head_tile_min", "e->n_pde <= e->fuse_seed_max",
                 "(b.n + 15) / 16 <= e->coop_fwd_max_tiles", "(b.n + 15) / 16 >= e->wide_min_tiles",
                 "e->main.n <= e->graph_max_points", "(b.n + 15) / 16 >= e->share_min_tiles * (int64_t)grid",
                 "(b.n + 15) / 16 >= 4 * e->share_min_tiles * (int64_t)grid", "dim3 g(head_grid(e, e->n_pde));", "dim3 g(head_grid(e, b.n));",
                 "fused_grid(e, e->main.n, 1, 2) <= HEAD_SLOTS", "fused_grid(e, e->main.n, 4, e->fwd_wg_per_cu) <= HEAD_SLOTS",
                 "(seed_in_reverse(e) || deep)", "cdiv(n, OBS_THREADS), OBS_MAX_WG)", "int64_t nchunk = (b.n + chunk - 1) / chunk;",
                 "(unsigned)((nchunk + 3) / 4)"):
        assert text in src, f"gpe_engine.hip no longer holds {text!r}: check the seam rows that rest on it"


def test_seams_at_256_cus():
    """the launched sizes at the MI355X's CU count"""
    at = {name: row["lower"](256) for name, row in S.SEAMS.items()}
    assert at == dict(bc_merge=39, wide_groups_round=128, gen_mfma_second_block=128, gen_mfma2_second_chunk=256, head_one_workgroup=1024,
                      wide256_groups_cap=2048, wide_fwd_grid_cap=4096, coop128_grid_cap=4096, fuse_head_max=6144, coop_grid_cap=8192,
                      graph_max_points=16384, gen_mfma2_chunk_grows=16640, wide_min_tiles=32752, coop_fwd_max_tiles=32768,
                      fuse_head_tile_min=32768, fuse_seed_max=65536, pipe_share=131056, gen_mfma_chunk_grows=131104, obs_grid_cap=262144,
                      head_grid_cap=262144, seed_grid_cap=262144, fwd_share=524272)
    # launched = bound + the merged boundary points, except where the condition counts collocation points
    assert S.bound_n(S.SEAMS["fuse_head_max"], 256) == 6139 and S.bound_n(S.SEAMS["fuse_seed_max"], 256) == 65536
    # the head can only move into f_forward once f_forward runs, and only while that kernel's capped grid fits HEAD_SLOTS
    assert S.SEAMS["fuse_head_tile_min"]["lower"](128) == 32768 and S.SEAMS["coop_fwd_max_tiles"]["lower"](128) == 16384
    assert S.SEAMS["fuse_head_tile_min"]["lower"](304) is None and S.SEAMS["coop_fwd_max_tiles"]["lower"](304) == 38912
    assert S.SEAMS["fuse_head_max"]["lower"](32) is None          # (6 144 points are past the cooperative forward there)
    # too few points to merge the boundary batch: launched = bound
    assert S.bound_n(S.SEAMS["wide_groups_round"], 256) == 123 and S.bound_n(S.SEAMS["bc_merge"], 256) == 39
    # H = 64 in 3D has no seed-forming reverse kernel, so its head never rides in f_forward_coop
    d3 = dict(S.CLASSES["NS"][1], dim=3)
    assert not S.SEAMS["fuse_head_max"]["applies_to"](d3) and S.SEAMS["fuse_head_max"]["applies_to"](dict(d3, maps=4))
    # the boundary points are merged at every seam (8 nb <= N), and every head-fusing grid fits the slots
    assert all(S.NB * S.D["merge_bc_ratio"] <= n for _, n, names in S.cells(256) if n > 200 and names != ["bc_merge"])
    assert min(S.D["fuse_head_max"] // S.TILE + 1, 2 * 256) <= S.D["HEAD_SLOTS"] and 2 * 256 <= S.D["HEAD_SLOTS"]


def test_every_row_is_well_formed():
    keys = {"origin", "lower", "counts", "visible", "applies_to", "below", "above", "cells", "note"}
    for name, row in S.SEAMS.items():
        assert set(row) <= keys and keys - {"below", "above"} <= set(row), (name, sorted(row))
        assert row["counts"] in ("launch", "pde", "obs") and row["note"].strip() and "\n" not in row["note"], name
        assert row["visible"] == ("below" in row) == ("above" in row), name
        assert row["cells"] and all(c in S.CLASSES and row["applies_to"](S.CLASSES[c][1]) for c in row["cells"]), name
        if row["visible"]:
            assert set(row["below"]) == set(row["above"]) and set(row["below"]) <= {"fwd", "bwd", "split"}, name
            for rx in list(row["below"].values()) + list(row["above"].values()):
                re.compile(rx)
    for cls, (kw, d) in S.CLASSES.items():
        layers, res = kw["layers"], kw.get("net_kind", 0) == go.NET_RESIDUAL
        assert d["H"] == max(layers[1:-1]) and d["dim"] == layers[0] and d["n_out"] == layers[-1] and d["res"] == res, cls
        assert d["path"] == ("generic" if cls in ("g512", "gres") else ("wide" if d["H"] >= 128 else "fused")), cls
        assert d["maps"] == (2 * (len(layers) - 3) if res else len(layers) - 3), cls


def test_expected_strings_of_both_sides():
    """the table's expressions on the strings gpe_active_kernels writes (formats of its snprintf calls)"""
    cu = 256
    lo = {"fwd": "f_forward_coop<32,4,1,1,1,head>", "bwd": "f_backward_pipe<32,4,1,1,1,seeds>", "split": "fwd 0/1024, bwd 0/1024"}
    assert not S.mismatches(lo, S.expected("A", 6139, cu))
    assert S.mismatches(lo, S.expected("A", 6140, cu))
    mid = dict(lo, fwd="f_forward_coop<32,4,1,1,1>")
    assert not S.mismatches(mid, S.expected("A", 6140, cu)) and not S.mismatches(mid, S.expected("A", 32763, cu))
    up = dict(lo, fwd="f_forward<32,4,1,1,wlds,head>")
    assert not S.mismatches(up, S.expected("A", 32764, cu)) and S.mismatches(mid, S.expected("A", 32764, cu))
    assert S.mismatches(dict(lo, fwd="f_forward<32,4,1,1,wlds>"), S.expected("A", 32764, cu))
    top = {"fwd": "f_forward<32,4,1,1,wlds,head>", "bwd": "f_backward_pipe<32,4,1,1,1>", "split": "fwd 640/1024, bwd 576/1024"}
    assert not S.mismatches(top, S.expected("A", 524268, cu)) and S.mismatches(top, S.expected("A", 524267, cu))
    assert S.mismatches(top, S.expected("A", 65536, cu)) and not S.mismatches(dict(top, split="fwd 0/1024, bwd 0/1024"), S.expected("A", 65537, cu))
    w = {"fwd": "f_forward_coop<128,4,1,1,1>", "bwd": "1 x w_bwd_map<128,4,1,1> (output layer fused into the top map)", "split": "fwd 0/1024, bwd 0/1024"}
    assert not S.mismatches(w, S.expected("w128", 32748, cu)) and S.mismatches(w, S.expected("w128", 32747, cu))


def fp32_blocks(pb, g32, g64):
    return H.block_rel_errs(g32, g64, H.param_blocks(pb.layers, pb.net_kind))


SEAM_CELLS = [(cls, n) for cls, n, _ in S.cells(256)]


@pytest.mark.parametrize("cls,n", SEAM_CELLS, ids=[f"{c}-{n}" for c, n in SEAM_CELLS])
def test_float32_oracle_meets_the_block_bound_on_both_sides_of_the_seam(cls, n):
    # (both sides where that is cheap; from 10^8 point-parameters on the upper side alone: one point more among thousands)
    for m in ((n + 1,) if n * go.param_count(R.problem(cls).layers, R.problem(cls).net_kind) > 1e8 else (n, n + 1)):
        sc64, g64 = R.step(cls, m, np.float64)
        sc32, g32 = R.step(cls, m, np.float32)
        errs = fp32_blocks(R.problem(cls), g32, g64)
        assert max(errs.values()) < FP32_BLOCK, (cls, m, errs)
        assert abs(sc32["mu"] - sc64["mu"]) < 2e-6 * abs(sc64["mu"]) and abs(sc32["loss"] - sc64["loss"]) < 1e-5 * abs(sc64["loss"]), (cls, m)


def _older_cells():
    from tests import test_gpu_parity as P
    from tests import test_gpu_switch_matrix as M
    out = []
    for name, (kw, N, _) in P.CASES.items():
        if N >= 4:                                    # (a single point: the bound carries the factor 10 of test_step_matches_oracle)
            out.append(pytest.param("parity", name, N, id=f"parity-{name}"))
    for name in M.CLASSES:
        for N, _, _ in M.CLASSES[name][1]:
            out.append(pytest.param("matrix", name, N, id=f"matrix-{name}-{N}"))
    return out


@pytest.mark.parametrize("table,name,N", _older_cells())
def test_float32_oracle_meets_the_block_bound_on_the_older_tables(table, name, N):
    """test_step_matches_oracle's CASES and the switch matrix's CLASSES, on the inputs those tests use"""
    from tests import test_gpu_parity as P
    from tests import test_gpu_switch_matrix as M
    if table == "parity":
        kw = P.CASES[name][0]
        x, flat, x_bc = P._inputs(kw, N, scale=P._scale(kw))
        orth = None
    else:
        kw = M.CLASSES[name][0]
        x, flat, x_bc, orth = M.inputs(name, N)
    pb = go.Problem(**kw)
    _, g64, _ = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), x_bc.astype(np.float64), orth=orth)
    _, g32, _ = go.full_loss_and_grad(pb, flat, x, x_bc, orth=orth)
    errs = fp32_blocks(pb, g32, g64)
    assert max(errs.values()) < FP32_BLOCK, (name, N, errs)
