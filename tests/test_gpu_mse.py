"""The value-only reverse pass -- the pre-training step bind_target / mse_loss_grad / mse_step -- against the float64 reference
tests/mse_ref.py, over every kernel family the (C = 1, E = 0) batch can launch: the shape table of tests/mse_cases.py on the fused and the
generic set, one cell per kernel switch that changes what the step launches, and the behaviour around the step (shards, bound weights and
boundary batch, leakage into the physics step, trajectories, repeatability, rebinding).

Bounds (none measured here): loss 1e-5 relative (test_mse_gradient_matches_oracle); gradient 5e-5 of max|g| and, per weight matrix and
bias, 5e-5 of that block's own maximum (test_step_matches_oracle, tests/test_gpu_dp_matrix.py).  tests/test_mse_reference_cpu.py shows the
float32 run of the reference below 1e-5 per block on every cell's inputs.

Measured on an MI355X (the module: 133 tests in 10 s on its own, references included; slowest cell 1.7 s, [3,256x6,1] at 4 099 points).  Largest gradient
error per reverse-kernel family, whole vector / worst block of its own maximum, beside the float32 reference's on the same cells.  (active_kernels
names the physics batch's kernels; the pre-training batch is selected by the same rules at C = 1 -- which differs in one place: H = 64 in
3D runs f_backward_coop at C = 5, whose two exchange buffers exceed the LDS, and f_backward_pipe<64,1,0> here.)
    f_backward_pipe<32|64> (1D, 2D and, at C = 1, 3D)   1.1e-6 / 3.5e-6   (float32 reference 6.7e-7 / 6.7e-7; [2,64x4,1] at 15 points, output bias)
    f_backward_coop<32|64> (4-5 maps, PIPE=0)     3.2e-7 / 4.1e-7   (2.6e-7 / 6.0e-7)
    f_backward_coop<.., RES>                      3.0e-7 / 3.3e-7   (1.5e-7 / 1.8e-7)
    f_backward_coop<.., B6>, f_forward_b6         2.0e-7 / 4.6e-7   (4.4e-8 / 3.9e-7)
    f_backward<32|64> (per wave; staged, unstaged, RACC=0)   2.0e-7 / 4.6e-7   (4.4e-8 / 3.9e-7)
    f_backward_coop<128> (also padded 100 -> 128) 2.7e-7 / 1.3e-6   (2.0e-7 / 3.3e-7)
    f_backward<128> on global-atomic slabs        1.0e-7 / 6.5e-7   (8.8e-8 / 1.9e-7)
    w_bwd_map<128> (w_forward, w_forward_mt, cooperative forward; with w_bwd_out)   1.8e-7 / 5.5e-7   (8.8e-8 / 1.9e-7)
    w_bwd_map<256>                                3.2e-7 / 4.8e-7   (2.8e-7 / 3.8e-7)
    g_bwd_weight (VALU)                           6.3e-7 / 1.2e-6   (7.3e-7 / 9.1e-7)
    g_bwd_weight_mfma                             1.1e-6 / 3.7e-6   (6.7e-7 / 6.7e-7)
    g_bwd_weight_mfma2                            3.4e-7 / 5.3e-7   (2.8e-7 / 3.8e-7)
Loss: 2.0e-6 at one point, below 3.2e-7 from 15 points on.  Every cell of the table is in and nothing is refused -- cfg4's network [2,128x6,2] runs on f_forward_coop<128> / f_backward_coop<128>.  No cell exposed a kernel fault: the
margin under 5e-5 is a factor 13 at the worst block.
Switch cells assert on active_kernels that their switch acted (SWITCH_CELLS); the rows that only move launch geometry or summation order
say beside them why they act at their size.  Not reachable: GPE_FWD_WG_PER_CU at fewer than 1 025 tiles (both caps are above the grid),
the uneven tile split below 2 048 tiles (it runs at 32 785 points with GPE_SHARE_MIN_TILES=1), GPE_WIDE=0 below wide_min_tiles.
"""
import os
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import Engine
from oracle import gpe_oracle as go
from tests import helpers as H
from tests import mse_cases as MC
from tests.mse_ref import mse_loss_and_grad
from tests.test_gpu_parity import PATHS, _inputs, _scale, cfg_from_problem
from tests.test_gpu_update_kernel import check_elements, ref_for, state

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL = 1e-5, 5e-5


@contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def kstr(k):
    return ";".join(f"{a}={b}" for a, b in k.items())


def bound_engine(pb, flat, x, target, **kw):
    """engine with parameters, points and target bound (no boundary batch, w_bc = 0)"""
    eng = Engine(cfg_from_problem(pb, **{"w_bc": 0.0, **kw}))
    try:
        eng.set_params(flat)
        eng.bind_points(dev(x))
        eng.bind_target(dev(target))
    except Exception:
        eng.close()
        raise
    return eng


def grad_failures(tag, loss, grad, ref_loss, ref_grad, blocks, f32=None):
    """prints every figure of the cell, then returns the checks it misses"""
    le = abs(loss - ref_loss) / ref_loss
    ge = H.rel_err(grad, ref_grad)
    blk = H.block_rel_errs(grad, ref_grad, blocks)
    wb = max(blk, key=blk.get)
    note = "" if f32 is None else f" | float32 reference: grad {f32['f32_whole']:.2e} worst block {max(f32['f32_blocks'].values()):.2e}"
    print(f"[mse] {tag} loss {le:.2e} grad {ge:.2e} worst block {wb} {blk[wb]:.2e}{note}")
    bad = []
    if not le < LOSS_TOL:
        bad.append(f"loss {loss!r} vs reference {ref_loss!r}: {le:.3e}")
    if not ge < GRAD_TOL:
        bad.append(f"gradient {ge:.3e} of max|g|")
    bad += [f"gradient block {nm}: {e:.3e} of its own maximum" for nm, e in blk.items() if not e < GRAD_TOL]
    return bad


def run_cell(name, N, path, env=None):
    """one engine under `env` (held for its life: some switches are read at launch): set_params, bind_points, bind_target, mse_loss_grad"""
    s = MC.setup(name, N)
    pb = s["pb"]
    with environment(env or {}):
        eng = bound_engine(pb, s["flat"], s["x"], s["target"], path=PATHS[path])
        try:
            assert eng.active_path == PATHS[path]
            kern = eng.active_kernels
            assert eng.n_params == go.param_count(pb.layers, pb.net_kind)           # padded widths: the caller's layout and count
            loss, grad = eng.mse_loss_grad()
            after = eng.get_params()
        finally:
            eng.close()
    assert grad.shape == (go.param_count(pb.layers, pb.net_kind),) and np.isfinite(grad).all()
    np.testing.assert_array_equal(after, s["flat"])                                 # mse_loss_grad does not update
    tag = f"{name} N={N} {path} {env or {}} -> {kstr(kern)}:"
    bad = grad_failures(tag, loss, grad, s["loss"], s["grad"], s["blocks"], s)
    assert not bad, tag + "\n" + "\n".join(bad[:30])
    return kern


# ---- the shape table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,path", MC.CELLS, ids=[f"{n}-N{N}-{p}" for n, N, p in MC.CELLS])
def test_mse_gradient_matches_reference(name, N, path):
    run_cell(name, N, path)


# ---- one cell per switch row that can change a kernel of the step ------------------------------------------------------------------------
# Each on the smallest table shape of the class the row applies to (tests/switch_table.py) at which the switch acts, and at 8 209 points
# (514 tiles: more than the persistent workgroups of one per CU) where it alters a multi-tile loop.  The update-form rows are here because
# the loss of the step is formed by the update kernel from the gradient buffer's tail.
#
# Last field, what the cell must show in active_kernels (which names the physics batch's kernels on the same points: the pre-training batch
# is selected by the same rules at C = 1) so that a cell its switch cannot reach does not stay green:
#   "differs"  another fwd / bwd / split string than the default engine's on the same cell (the switch matrix's rule for its "kernels" rows)
#   "same"     the side of a threshold, or the network class, where the switch must NOT move the kernels
#   a string   that text appears (the uneven tile split reports its shares)
#   "order"    only launch geometry or summation order changes, nothing to read back: why it acts at this size is beside the row
S32, S64, L64, H128, W256, R64, P100 = (("1d_32x2", 333), ("2d_64x4", 333), ("2d_64x4_large", 8209), ("2d_128x3", 300), ("3d_256x2", 300),
                                        ("1d_res_64x2blocks", 300), ("2d_100x3_pads_to_128", 300))
H128L, H128XL, XL64 = ("2d_128x3", 4113), ("2d_128x3_large", 32785), ("2d_64x4_large", 32785)
BIG = "1000000000"
# 32 785 points = 2 050 tiles: the per-wave forward runs on min(513, 2 num_cu) workgroups and the pipelined reverse kernel on min(2 050,
# 2 num_cu); with 256 CUs both grids are 2 num_cu and GPE_SHARE_MIN_TILES=1 puts both above their thresholds (4 x 512 and 512 tiles), so the
# uneven split of a CU's tiles between its two workgroups runs in f_forward<64,1,0> and f_backward_pipe<64,1,0> (about eight tiles per CU:
# 576 / 700 of 1024 and the even split place tiles differently).  GPE_FUSE_SEED_MAX=0 only makes the physics batch report its reverse share.
SHARE = {"GPE_SHARE_MIN_TILES": "1", "GPE_FUSE_SEED_MAX": "0"}
SWITCH_CELLS = [
    ("GPE_COOP", {"GPE_COOP": "0"}, [S32, L64, H128], "fused", "differs"),
    ("GPE_COOP-residual", {"GPE_COOP": "0"}, [R64], "fused", "same"),          # residual blocks keep the cooperative kernels
    ("GPE_COOP+STAGE_MIN_TILES", {"GPE_COOP": "0", "GPE_STAGE_MIN_TILES": BIG}, [S32, L64], "fused", "differs"),
    ("GPE_COOP+WLDS", {"GPE_COOP": "0", "GPE_WLDS": "0"}, [S32, L64], "fused", "differs"),
    ("GPE_WLDS", {"GPE_WLDS": "0", "GPE_COOP_FWD_MAX_TILES": "0"}, [S32, L64], "fused", "differs"),
    ("GPE_COOP+RACC", {"GPE_COOP": "0", "GPE_RACC": "0"}, [S32, L64], "fused", "differs"),
    ("GPE_COOP=-1", {"GPE_COOP": "-1"}, [S32, L64], "fused", "differs"),
    ("GPE_PIPE", {"GPE_PIPE": "0"}, [S32, L64], "fused", "differs"),
    ("GPE_BWD_B6", {"GPE_BWD_B6": "1"}, [S32, L64], "fused", "differs"),
    ("GPE_BWD_B6+FWD_B6", {"GPE_BWD_B6": "1", "GPE_FWD_B6": "1", "GPE_COOP_FWD_MAX_TILES": "0"}, [S32, L64], "fused", "differs"),
    ("GPE_FWD_B6", {"GPE_FWD_B6": "1", "GPE_COOP_FWD_MAX_TILES": "0"}, [S32, L64], "fused", "differs"),
    ("GPE_FWD_B6+COOP", {"GPE_COOP": "0", "GPE_FWD_B6": "1"}, [S32, L64], "fused", "differs"),
    ("GPE_COOP128", {"GPE_COOP128": "0", "GPE_WIDE": "0"}, [H128, H128L], "fused", "differs"),
    ("GPE_COOP_FWD128", {"GPE_COOP_FWD128": "0"}, [H128, H128L], "fused", "differs"),
    ("GPE_COOP_MAX_TILES=64-below", {"GPE_COOP": "-1", "GPE_COOP_MAX_TILES": "64"}, [S32], "fused", "same"),      # 21 tiles: still cooperative
    ("GPE_COOP_MAX_TILES=64", {"GPE_COOP": "-1", "GPE_COOP_MAX_TILES": "64"}, [L64], "fused", "differs"),
    ("GPE_COOP_MAX_TILES=1", {"GPE_COOP": "2", "GPE_COOP_MAX_TILES": "1"}, [S32, L64], "fused", "differs"),
    ("GPE_COOP_FWD_MAX_TILES", {"GPE_COOP_FWD_MAX_TILES": "0"}, [S32, L64], "fused", "differs"),
    # 514 tiles on 256 persistent workgroups instead of 512
    ("GPE_COOP_WG_PER_CU", {"GPE_COOP_WG_PER_CU": "1"}, [L64], "fused", "order"),
    # 513 workgroups' worth of tiles on 256 workgroups instead of 512 (at 8 209 points the 129 workgroups are below both caps: no cell)
    ("GPE_FWD_WG_PER_CU", {"GPE_FWD_WG_PER_CU": "1"}, [XL64], "fused", "order"),
    ("GPE_SHARE_MIN_TILES", SHARE, [XL64], "fused", "split=fwd 640/1024, bwd 576/1024"),
    ("GPE_PIPE_SHARE=0", dict(SHARE, GPE_PIPE_SHARE="0"), [XL64], "fused", "split=fwd 640/1024, bwd 0/1024"),
    ("GPE_PIPE_SHARE=700", dict(SHARE, GPE_PIPE_SHARE="700"), [XL64], "fused", "split=fwd 640/1024, bwd 700/1024"),
    ("GPE_FWD_SHARE=0", dict(SHARE, GPE_FWD_SHARE="0"), [XL64], "fused", "split=fwd 0/1024, bwd 576/1024"),
    ("GPE_FWD_SHARE=300", dict(SHARE, GPE_FWD_SHARE="300"), [XL64], "fused", "split=fwd 300/1024, bwd 576/1024"),
    # below wide_min_tiles the default is the cooperative pair already: GPE_WIDE=0 acts from 2 048 tiles on
    ("GPE_WIDE=0-below", {"GPE_WIDE": "0"}, [H128], "fused", "same"),
    ("GPE_WIDE=0", {"GPE_WIDE": "0"}, [H128XL], "fused", "differs"),
    ("GPE_WIDE=1", {"GPE_WIDE": "1", "GPE_WIDE_MIN_TILES": "0"}, [H128, H128L], "fused", "differs"),
    ("GPE_WIDE_MIN_TILES", {"GPE_WIDE_MIN_TILES": "0"}, [H128, H128L], "fused", "differs"),
    # read at every launch of the wide reverse pass: w_bwd_out in a launch of its own (active_kernels cannot know)
    ("GPE_WIDE_TOP", {"GPE_WIDE_TOP": "0"}, [W256], "fused", "order"),
    ("GPE_WIDE_TOP+MIN_TILES", {"GPE_WIDE_TOP": "0", "GPE_WIDE_MIN_TILES": "0"}, [H128, H128L], "fused", "differs"),
    ("GPE_PAD_WIDTH", {"GPE_PAD_WIDTH": "0"}, [P100], "generic", "auto"),
    ("GPE_RES_FUSED", {"GPE_RES_FUSED": "0"}, [R64], "generic", "auto"),
    ("GPE_GEN_MFMA", {"GPE_GEN_MFMA": "0"}, [S64, W256], "generic", "differs"),          # (width 32 has no matrix-core kernel to lose)
    ("GPE_GEN_MFMA2", {"GPE_GEN_MFMA2": "0"}, [H128, W256], "generic", "differs"),       # (widths that are multiples of 128 / 256 only)
    # split-K chunk of the weight gradient: 333 points are 11 chunks of 32 by default, 2 of 256 or 21 of 16 here
    ("GPE_GEN_MIN_CHUNK=256", {"GPE_GEN_MIN_CHUNK": "256"}, [S64, W256], "generic", "order"),
    ("GPE_GEN_MIN_CHUNK=16", {"GPE_GEN_MIN_CHUNK": "16"}, [S64], "generic", "order"),
    # forms of the update kernel (12 737 parameters: cached single-workgroup form by default; 33 537: multi-workgroup by default)
    ("GPE_UPDATE_CACHE", {"GPE_UPDATE_CACHE": "0"}, [S64], "fused", "order"),
    ("GPE_FUSE_UPDATE", {"GPE_FUSE_UPDATE": "1"}, [S64], "fused", "order"),
    ("GPE_SPLIT_UPDATE", {"GPE_SPLIT_UPDATE": "1"}, [S64], "fused", "order"),
    ("GPE_UPDATE_MULTI_MIN", {"GPE_UPDATE_MULTI_MIN": "1"}, [S64], "fused", "order"),
    ("GPE_UPDATE_MULTI", {"GPE_UPDATE_MULTI": "0"}, [H128], "fused", "order"),
]


def _switch_params():
    return [pytest.param(tag, env, name, N, path, expect, id=f"{tag}-{name}-N{N}")
            for tag, env, shapes, path, expect in SWITCH_CELLS for name, N in shapes]


_DEFAULT_KERNELS = {}


def default_kernels(name, N, path):
    """active_kernels of the default engine on the cell's points (binding is enough to read the names: no step)"""
    key = (name, N, path)
    if key not in _DEFAULT_KERNELS:
        s = MC.setup(name, N)
        eng = bound_engine(s["pb"], s["flat"], s["x"], s["target"], path=PATHS[path])
        try:
            _DEFAULT_KERNELS[key] = kstr(eng.active_kernels)
        finally:
            eng.close()
    return _DEFAULT_KERNELS[key]


@pytest.mark.parametrize("tag,env,name,N,path,expect", _switch_params())
def test_mse_gradient_under_kernel_switches(tag, env, name, N, path, expect):
    if expect == "auto":          # the switch moves the network from the fused to the generic set: gpe_create chooses
        s = MC.setup(name, N)
        with environment(env):
            eng = bound_engine(s["pb"], s["flat"], s["x"], s["target"])
            try:
                assert eng.active_path == gpe_pinn.PATH_GENERIC, kstr(eng.active_kernels)
                loss, grad = eng.mse_loss_grad()
                kern = eng.active_kernels
            finally:
                eng.close()
        bad = grad_failures(f"{name} N={N} auto {env} -> {kstr(kern)}:", loss, grad, s["loss"], s["grad"], s["blocks"], s)
        assert not bad, "\n".join(bad[:30])
        return
    kern = kstr(run_cell(name, N, path, env))
    if expect == "differs":
        assert kern != default_kernels(name, N, path), f"{tag}: the switch selected what runs by default on this cell -- dead cell: {kern}"
    elif expect == "same":
        assert kern == default_kernels(name, N, path), f"{tag}: {kern} != default {default_kernels(name, N, path)}"
    elif expect != "order":
        assert expect in kern, f"{tag}: expected {expect!r} in {kern} (the uneven split needs grids of 2 num_cu workgroups)"


def wide_mt_child():
    """the cells of GPE_WIDE_FWD_MT=1 (read once per process by the wide unit): run by test_wide_multi_tile_forward_in_a_child_process"""
    assert os.environ.get("GPE_WIDE_FWD_MT") == "1"
    for name, N in (H128, H128L, W256):
        kern = kstr(run_cell(name, N, "fused"))
        print(kern, flush=True)
        assert ("w_forward_mt<" in kern) == (name == H128[0]), kern          # (H = 128 only: H = 256 keeps w_forward)


def test_wide_multi_tile_forward_in_a_child_process():
    """GPE_WIDE=1 GPE_WIDE_FWD_MT=1: the wide set's multi-tile forward kernel storing for the value-only reverse pass; one child process
    for all its cells, since the switch is read once per process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GPE_WIDE="1", GPE_WIDE_FWD_MT="1", GPE_WIDE_MIN_TILES="0")
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_mse import wide_mt_child; wide_mt_child()"], capture_output=True,
                       text=True, timeout=300, cwd=root, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


# ---- behaviour around the step -----------------------------------------------------------------------------------------------------------
BKW = dict(layers=[2, 64, 64, 64, 1], gamma=50.0, dx=0.01)
_BSETUP = {}


def bsetup(N):
    """[2,64,64,64,1] with a physics problem around it (the step() calls of the leakage tests), N points, reference computed once"""
    if N not in _BSETUP:
        pb = go.Problem(**BKW, w_bc=0.0)
        x, flat, x_bc = _inputs(BKW, N, scale=_scale(BKW))
        target = MC.target_of(x, 1).astype(np.float32)
        loss, grad = mse_loss_and_grad(pb, flat, x, target)
        _BSETUP[N] = dict(pb=pb, x=x, flat=flat, x_bc=x_bc, target=target, loss=loss, grad=grad, blocks=H.param_blocks(pb.layers))
    return _BSETUP[N]


@pytest.mark.parametrize("N", [333, 8209])
def test_two_shards_add_up_to_the_reference(N):
    """two engines with world_size = 2 and n_global = N on rows 0..17 and 17..N: their losses and gradients, added in float64, are the
    one-set reference (each shard divides by n_global, not by its own count)"""
    s = bsetup(N)
    loss, grad = 0.0, np.zeros(s["grad"].size)
    for lo, hi in ((0, 17), (17, N)):
        eng = bound_engine(s["pb"], s["flat"], s["x"][lo:hi], s["target"][lo:hi], world_size=2, n_global=N)
        try:
            l, g = eng.mse_loss_grad()
        finally:
            eng.close()
        rl, rg = mse_loss_and_grad(s["pb"], s["flat"], s["x"][lo:hi], s["target"][lo:hi], n_global=N)
        assert abs(l - rl) < LOSS_TOL * rl and H.rel_err(g, rg) < GRAD_TOL, (lo, hi)
        loss += l
        grad += g.astype(np.float64)
    bad = grad_failures(f"two shards N={N}:", loss, grad, s["loss"], s["grad"], s["blocks"])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("N", [333, 8209])
def test_bound_weights_and_merged_boundary_leave_the_mse_step_alone(N):
    """the pre-training loss is unweighted and runs on the collocation rows only: with quadrature weights and a 5-point boundary batch
    (merged into the collocation launch) bound, mse_loss_grad returns the bare engine's bits"""
    s = bsetup(N)
    pb = go.Problem(**BKW)                                         # w_bc = 10: the boundary batch is live
    q = np.random.default_rng(11).uniform(0.2, 3.0, N).astype(np.float32)
    out = []
    for dressed in (False, True):
        eng = Engine(cfg_from_problem(pb))
        try:
            eng.set_params(s["flat"])
            eng.bind_points(dev(s["x"]))
            if dressed:
                eng.bind_boundary(dev(s["x_bc"]))
                eng.bind_weights(dev(q))
            eng.bind_target(dev(s["target"]))
            out.append(eng.mse_loss_grad())
            if dressed:
                sc = eng.step()                                    # ... and the weights and the boundary batch are indeed bound
                assert sc["bc"] > 0 and abs(eng.weights()["total"] - float(q.astype(np.float64).sum())) < 1e-6 * q.sum()
        finally:
            eng.close()
    assert out[0][0] == out[1][0]
    np.testing.assert_array_equal(out[0][1], out[1][1])
    bad = grad_failures(f"weights + boundary bound N={N}:", out[1][0], out[1][1], s["loss"], s["grad"], s["blocks"])
    assert not bad, "\n".join(bad)


def _full_state(eng):
    th, m, v, step = state(eng)
    return dict(theta=th, m=m, v=v, step=step, sc=eng.read_scalars(), grad=eng.get_grad())


# head inside the forward kernel: the plain real-psi class at 4 000 points.  GPE_FUSE_HEAD=0: k_head_pde, at 333 points -- one head
# workgroup, so its double-precision atomics add in one order and the step is reproducible bit for bit (above 1 024 points it is not)
@pytest.mark.parametrize("env,N", [({}, 4000), ({"GPE_FUSE_HEAD": "0"}, 333)], ids=["head_in_forward_N4000", "GPE_FUSE_HEAD=0_N333"])
def test_mse_loss_grad_leaves_nothing_behind_in_the_physics_step(env, N):
    """step(); mse_loss_grad(); step() on one engine against step(); step() on another: parameters, Adam state, gradient and every scalar
    of the second step bit-identical"""
    s = bsetup(N)
    got = []
    with environment(env):
        for with_mse in (True, False):
            eng = bound_engine(s["pb"], s["flat"], s["x"], s["target"])
            try:
                kern = eng.active_kernels
                first = eng.step()
                if with_mse:
                    before = eng.get_params()
                    loss, grad = eng.mse_loss_grad()
                    np.testing.assert_array_equal(eng.get_params(), before)
                    rl, rg = mse_loss_and_grad(s["pb"], before, s["x"], s["target"])
                    bad = grad_failures(f"between two steps N={N} {env}:", loss, grad, rl, rg, s["blocks"])
                    assert not bad, "\n".join(bad)
                eng.step()
                got.append((first, _full_state(eng)))
            finally:
                eng.close()
    print(f"[mse] leakage {env} N={N}: {kstr(kern)}")
    assert kern["fwd"].endswith(",head>") == (not env), kern          # the head inside the forward kernel, or (GPE_FUSE_HEAD=0) in k_head_pde
    (fa, a), (fb, b) = got
    assert fa == fb
    assert a["step"] == b["step"] == 2
    for k in ("theta", "m", "v", "grad"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["sc"] == b["sc"], {k: (a["sc"][k], b["sc"][k]) for k in a["sc"] if a["sc"][k] != b["sc"][k]}


def test_mse_step_between_two_steps_follows_the_float64_chain():
    """step(); mse_step(); step() against the float64 chain oracle step, plain-Adam MSE step (no clipping, no scheduler), oracle step on one
    Adam state -- at the trajectory tolerances of tests/test_oracle_golden.py (loss and gradient norm 2e-3, mu 5e-4); the first step at
    those of test_step_matches_oracle.  The bound on the parameters after the chain is this test's own, not a golden tolerance:
    test_step_matches_oracle allows one Adam step q99 < 2e-5 and max < 2.1e-3 (+-lr where a gradient element near zero flips Adam's sign),
    and three steps can each add that much, so three times both."""
    N = 333
    s = bsetup(N)
    pb, x64 = s["pb"], s["x"].astype(np.float64)
    eng = bound_engine(pb, s["flat"], s["x"], s["target"])
    try:
        ref = ref_for(eng)
        scs = [eng.step(), eng.mse_step(), eng.step()]
        params = eng.get_params()
        _, _, step = eng.get_adam_state()
    finally:
        eng.close()
    want = []
    for kind in ("pde", "mse", "pde"):
        if kind == "pde":
            osc, og, _ = go.full_loss_and_grad(pb, ref.theta, x64)
            r = ref.update(og, osc["loss"])
            want.append(dict(loss=osc["loss"], mu=osc["mu"], grad_norm=r["grad_norm"]))
        else:
            l, g = mse_loss_and_grad(pb, ref.theta, s["x"], s["target"])
            r = ref.update(g, l, mse_mode=True)
            assert r["coef"] == 1.0
            want.append(dict(loss=l, mu=0.0, grad_norm=r["grad_norm"]))
    assert step == ref.step == 3 and [sc["step"] for sc in scs] == [1, 2, 3]
    for k, (sc, w) in enumerate(zip(scs, want)):
        print(f"[mse] chain step {k}: loss {abs(sc['loss'] - w['loss']) / w['loss']:.2e} mu {abs(sc['mu'] - w['mu']):.2e} "
              f"grad_norm {abs(sc['grad_norm'] - w['grad_norm']) / w['grad_norm']:.2e}")
    assert abs(scs[0]["loss"] - want[0]["loss"]) <= 1e-4 * want[0]["loss"] and abs(scs[0]["mu"] - want[0]["mu"]) <= 2e-5 * abs(want[0]["mu"])
    for sc, w in zip(scs, want):
        assert abs(sc["loss"] - w["loss"]) <= 2e-3 * w["loss"]
        assert abs(sc["grad_norm"] - w["grad_norm"]) <= 2e-3 * w["grad_norm"]
        assert abs(sc["mu"] - w["mu"]) <= 5e-4 * abs(w["mu"])
    assert scs[1]["mu"] == 0.0 and scs[1]["pde"] == 0.0
    d = np.abs(params - ref.theta)
    print(f"[mse] chain parameters: q99 {np.quantile(d, 0.99):.2e} max {d.max():.2e}")
    assert np.quantile(d, 0.99) < 3 * 2e-5 and d.max() < 3 * 2.1e-3


def test_five_mse_steps_against_the_reference_trajectory():
    """five mse_step calls.  Per step: the engine's gradient at its own parameters against the reference's there (5e-5, whole and per
    block), and the update against oracle/update_ref.py in mse_mode fed the engine's fp32 state and that gradient, element by element
    within the round-off bounds of tests/test_gpu_update_kernel.py.  Beside it the free-running float64 trajectory (reference gradient
    into update_ref from the start parameters): the recorded loss of every step at the trajectory tolerance 2e-3 of
    tests/test_oracle_golden.py."""
    N = 333
    s = bsetup(N)
    pb = s["pb"]
    eng = bound_engine(pb, s["flat"], s["x"], s["target"])
    try:
        ref, free = ref_for(eng), ref_for(eng)
        for k in range(5):
            th0, m0, v0, step0 = state(eng)
            ref.theta, ref.m, ref.v = th0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
            assert step0 == ref.step == k
            sc = eng.mse_step()
            g = eng.get_grad()
            rl, rg = mse_loss_and_grad(pb, th0, s["x"], s["target"])
            bad = grad_failures(f"mse_step {k}:", sc["loss"], g, rl, rg, s["blocks"])
            assert not bad, "\n".join(bad)
            r = ref.update(g, sc["loss"], mse_mode=True)
            assert r["status"] == "applied" and r["coef"] == 1.0
            gn = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
            assert abs(sc["grad_norm"] - gn) <= 1e-10 * gn and sc["step"] == k + 1 and sc["lr"] == ref.lr0
            check_elements(state(eng), r, m0.astype(np.float64), f"mse_step {k}")
            fl, fg = mse_loss_and_grad(pb, free.theta, s["x"], s["target"])
            free.update(fg, fl, mse_mode=True)
            print(f"[mse] mse_step {k}: loss off the free-running float64 trajectory by {abs(sc['loss'] - fl) / fl:.2e}")
            assert abs(sc["loss"] - fl) <= 2e-3 * fl
        hist = eng.read_history(1, 5)
        assert [int(h["step"]) for h in hist] == [1, 2, 3, 4, 5]
        assert hist[-1]["loss"] < hist[0]["loss"]
    finally:
        eng.close()


# Repeatability is asserted on the default kernels only.  Left out, with the README's word that they sum with atomics in arrival order:
# the generic set at widths that are multiples of 64 (split-K weight gradient, global atomics) and the per-wave reverse kernels
# (GPE_COOP=0: LDS atomics across waves).
@pytest.mark.parametrize("N", [333, 8209])
def test_mse_gradient_repeats_bit_for_bit_on_the_default_kernels(N):
    s = bsetup(N)
    out = []
    for _ in range(2):
        eng = bound_engine(s["pb"], s["flat"], s["x"], s["target"])
        try:
            assert eng.active_path == gpe_pinn.PATH_FUSED
            out += [eng.mse_loss_grad(), eng.mse_loss_grad()]
        finally:
            eng.close()
    for l, g in out[1:]:
        assert l == out[0][0]
        np.testing.assert_array_equal(g, out[0][1])


def test_rebinding_points_and_targets():
    s, s2 = bsetup(333), bsetup(8209)
    pb = s["pb"]
    big_loss, big_grad = mse_loss_and_grad(pb, s["flat"], s2["x"], s2["target"])          # the engine keeps the parameters of the small set
    eng = bound_engine(pb, s["flat"], s["x"], s["target"])
    try:
        eng.mse_loss_grad()
        # 1. no target: the step is refused, nothing moves
        eng.bind_target(None)
        with pytest.raises(gpe_pinn.GPEError) as ei:
            eng.mse_step()
        assert ei.value.code == gpe_pinn.capi.GPE_ERR_STATE and "bind_target" in str(ei.value)
        np.testing.assert_array_equal(eng.get_params(), s["flat"])
        # 2. other points (another N: other tile counts, other kernels' grids), then the target of those points
        eng.bind_points(dev(s2["x"]))
        with pytest.raises(gpe_pinn.GPEError) as ei:          # the old target went with the old points
            eng.mse_step()
        assert ei.value.code == gpe_pinn.capi.GPE_ERR_STATE
        eng.bind_target(dev(s2["target"]))
        loss, grad = eng.mse_loss_grad()
        bad = grad_failures("rebound to N=8209:", loss, grad, big_loss, big_grad, s["blocks"])
        assert not bad, "\n".join(bad)
        # ... and back to the small set
        eng.bind_points(dev(s["x"]))
        first_target = dev(s["target"])          # (kept here: the array stays alive while the new one is made, so the pointers differ)
        eng.bind_target(first_target)
        loss, grad = eng.mse_loss_grad()
        bad = grad_failures("rebound to N=333:", loss, grad, s["loss"], s["grad"], s["blocks"])
        assert not bad, "\n".join(bad)
        # 3. same points, a new target array
        t2 = (0.25 - s["target"][::-1]).astype(np.float32)
        new = dev(t2)
        assert new.data_ptr() != first_target.data_ptr()
        eng.bind_target(new)
        loss, grad = eng.mse_loss_grad()
        rl, rg = mse_loss_and_grad(pb, s["flat"], s["x"], t2)
        assert H.rel_err(rg, s["grad"]) > 1000 * GRAD_TOL          # (the old target's gradient would miss the bound by far)
        bad = grad_failures("new target array:", loss, grad, rl, rg, s["blocks"])
        assert not bad, "\n".join(bad)
    finally:
        eng.close()
