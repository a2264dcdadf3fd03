"""The cell-subset sampler (include/gpe_hip.h: gpe_sampler_cells; csrc/gpe_sampler.h: k_sampler_draw_cells / k_sampler_draw_graded_cells)
on the device: its sets against the numpy restatement gpe_pinn.sampler.cells_points / cells_weights / cells_total bit for bit, the full
list against the plain and the graded sampler bit for bit, blocks of rows, one step against the fp64 oracle (tolerances of
tests/test_gpu_sampler.py for the uniform form, of tests/test_gpu_weights.py for the graded form, of tests/test_gpu_mixture.py for the
mixture), graph replay, three ranks by hand, the frozen orthogonality state, the symmetry batch, replacing / clearing, and the refusals.

The shapes are the smallest at which the indirection can go wrong: 1D 16 cells with the list [0, 1, 5, 6, 7, 15]; 2D 12 x 10 cells with
the disk of radius 2; 3D 6 x 5 x 4 cells with the ball of radius 2.  At these sizes every sum of a step is added in a fixed order
(README, Reproducibility), which is what the bit-for-bit comparisons of two engines lean on."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpe_pinn import Engine, GPEError, capi
from gpe_pinn import sampler as S
from oracle import gpe_oracle as go
from tests import helpers as H
from tests import mixture_cases as mc
from tests import mixture_ref as mr
from tests.test_gpu_dp_matrix import dp_step
from tests.test_gpu_mixture import config as mix_config, environment, failures as mix_failures, record as mix_record
from tests.test_gpu_orth_states import _frozen, _oracle_psi
from tests.test_gpu_parity import CASES, _inputs, cfg_from_problem, close
from tests.test_gpu_weights import check_scalars
from tests.weighted_ref import weighted_loss_and_grad

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15                            # a non-zero high word
GRID = {1: dict(lo=(-6.0,), hi=(6.0,), shape=(16,)),
        2: dict(lo=(-3.0, -2.5), hi=(3.0, 2.5), shape=(12, 10)),
        3: dict(lo=(-3.0, -2.5, -2.0), hi=(3.0, 2.5, 2.0), shape=(6, 5, 4))}
EDGES = {1: [S.sinh_edges(6.0, 16, 2.0)], 2: [S.sinh_edges(3.0, 12, 2.5), S.sinh_edges(2.5, 10, 1.0)],
         3: [S.sinh_edges(3.0, 6, 1.5), S.sinh_edges(2.5, 5, 2.0), S.sinh_edges(2.0, 4, 0.5)]}
LIST = {1: np.array([0, 1, 5, 6, 7, 15], dtype=np.int64), 2: S.ball_cells(radius=2.0, **GRID[2]), 3: S.ball_cells(radius=2.0, **GRID[3])}
DISK = LIST[2]
VOL = {d: float(np.prod([(h - l) / s for l, h, s in zip(GRID[d]["lo"], GRID[d]["hi"], GRID[d]["shape"])])) for d in GRID}
# the uniform step's bars (tests/test_gpu_sampler.py: test_step_after_a_redraw_matches_oracle)
UNIFORM_TOLS = (("mu", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("bc", 1e-4), ("norm", 2e-4), ("sym", 1e-4), ("riesz", 1e-4), ("reg", 1e-4))


def test_the_lists_are_what_the_issue_names():
    assert 19 <= DISK.size <= 64 and 0 < LIST[3].size < 120          # (three ranks on cuts (1, 17, K - 18); a graph-replay case of <= 64 points)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def code(fn, *a, **k):
    with pytest.raises(GPEError) as ex:
        fn(*a, **k)
    return ex.value.code


def small_engine(d, width=32, **kw):
    """a real-psi network on d axes with fixed parameters; dx = 1 (graded binds) unless given"""
    cfg = dict(layers=[d, width, width, 1], gamma=20.0, dx=1.0, w_bc=0.0)
    cfg.update(kw)
    pb = go.Problem(**cfg)
    flat = (np.random.default_rng(21).normal(0, 1, go.param_count(cfg["layers"])) * 0.3).astype(np.float32)
    eng = Engine(cfg_from_problem(pb, sched=capi.SCHED_CONST))
    eng.set_params(flat)
    return eng, pb, flat


def state(eng):
    m, v, step = eng.get_adam_state()
    return eng.get_params(), m, v, step


def same_state(a, b):
    return all(same(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]


def want_points(d, graded, draw, cells=None, clip=None):
    cells = LIST[d] if cells is None else cells
    return S.cells_points(cells, seed=SEED, draw=draw, clip=clip, edges=EDGES[d] if graded else None, **GRID[d])


# ---- 1. the device set is cells_points, bit for bit, at the bind and behind every redraw ---------------------------------------------
@pytest.mark.parametrize("graded", [False, True], ids=["uniform", "graded"])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_device_set_equals_the_restatement_bit_for_bit(d, graded):
    every, draw0 = 4, 2 ** 33 + 3
    clip = None if d != 2 else ((-2.9, -2.4), (2.9, 2.4))
    eng, _, _ = small_engine(d, dx=1.0 if graded else VOL[d])
    eng.bind_sampler_cells(LIST[d], every=every, seed=SEED, draw0=draw0, clip=clip, edges=EDGES[d] if graded else None, **GRID[d])
    total = 0
    for chunk in (0, 1, every - 2, 1, every + 1):          # 0, 1, every - 1, every and 2 * every + 1 steps since the bind
        if chunk:
            eng.run(chunk)
        total += chunk
        pts, draw = eng.sampler_points()
        assert draw == draw0 + (max(total, 1) - 1) // every, (total, draw)
        assert tuple(pts.shape) == (LIST[d].size, d) and same(pts, want_points(d, graded, draw, clip=clip)), (d, graded, total)
        if graded:
            w = eng.weights()
            q = S.cells_weights(LIST[d], EDGES[d])
            assert same(w["q"], q) and w["total"] == S.cells_total(LIST[d], EDGES[d])
            assert abs(w["local"] - q.sum(dtype=np.float64)) <= 1e-12 * w["total"]
        else:
            assert code(eng.weights) == capi.GPE_ERR_STATE
    assert total == 2 * every + 1
    cells, first = eng.sampler_cells()
    assert first == 0 and cells.dtype == np.int64 and np.array_equal(cells, LIST[d])
    assert code(eng.adaptive_state) == capi.GPE_ERR_STATE          # as with no adaptive sampler bound
    eng.close()


# ---- 1b. each of the four grid kernels x dim x a ragged row count x a non-zero first row, at the bind and behind a redraw -------------
# 4 099 rows: 16 full workgroups of 256 and a ragged tail; 17: one ragged workgroup; 1: the degenerate set.  The bind's launch writes the
# graded weights (qw given), the redraw's does not (qw NULL).  "+sym": the two uniform forms with w_sym != 0, whose launch writes the
# [x ; -x] batch as well (xs given).  The engine does not expose that batch; the step's sym term reads nothing else, so it is held to the
# oracle on [x ; -x] of the restated set, with the bar of test_the_symmetry_batch_follows_the_redraw (UNIFORM_TOLS).
MATRIX_SHAPE = {1: (5003,), 2: (17, 301), 3: (36, 13, 11)}                  # last axes no powers of two; 6 / 7 of the cells >= 29 + 4 099
MATRIX_KERNELS = ["k_sampler_draw", "k_sampler_draw_graded", "k_sampler_draw_cells", "k_sampler_draw_graded_cells", "k_sampler_draw+sym",
                  "k_sampler_draw_cells+sym"]


@pytest.mark.parametrize("N", [1, 17, 4099])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("kernel", MATRIX_KERNELS)
def test_every_grid_kernel_holds_the_restatement_at_the_bind_and_behind_a_redraw(kernel, d, N):
    graded, listed, sym = "graded" in kernel, "cells" in kernel, kernel.endswith("+sym")
    half, shape = (3.0, 2.5, 2.0)[:d], MATRIX_SHAPE[d]
    lo, hi = tuple(-h for h in half), half
    ed = [S.sinh_edges(h, s, 1.5) for h, s in zip(half, shape)]
    total = int(np.prod(shape))
    cells = np.flatnonzero(np.arange(total) % 7 != 3).astype(np.int64)         # a list with gaps
    first, seed, draw0 = 29, SEED, 2 ** 33 + 1
    assert first + N <= cells.size
    eng, pb, _ = small_engine(d, dx=1.0, **(dict(w_sym=5.0) if sym else {}))
    if listed:
        eng.bind_sampler_cells(cells, lo, hi, shape, every=1, seed=seed, draw0=draw0, edges=ed if graded else None, first=first, n_local=N)
        rows = cells[first:first + N]
    else:
        if graded:
            eng.bind_sampler_graded(ed, every=1, seed=seed, draw0=draw0, first_cell=first, n=N)
        else:
            eng.bind_sampler(lo, hi, shape, every=1, seed=seed, draw0=draw0, first_cell=first, n=N)
        rows = np.arange(first, first + N, dtype=np.int64)
    q = S.cells_weights(rows, ed) if graded else None

    def held(step):
        """the buffer holds the restated set of draw0 + step (and the graded weights); -> that set"""
        pts, draw = eng.sampler_points()
        assert draw == draw0 + step and tuple(pts.shape) == (N, d)
        if listed:
            want = S.cells_points(rows, lo, hi, shape, seed, draw, edges=ed if graded else None)
        elif graded:
            want = S.graded_points(ed, seed, draw, first_cell=first, n=N)
        else:
            want = S.stratified_points(lo, hi, shape, seed, draw, first_cell=first, n=N)
        assert same(pts, want), (kernel, d, N, step)
        if graded:
            assert same(eng.weights()["q"], q), (kernel, d, N, step)
        return want

    ran = []                                             # (parameters, scalars, set) of the step on the bind's draw and of the one behind the redraw
    flat0, x0 = eng.get_params(), held(0)
    ran.append((flat0, eng.step(), x0))
    flat1 = eng.get_params()
    sc1 = eng.step()                                     # every = 1: starts with the redraw
    ran.append((flat1, sc1, held(1)))
    if sym:
        for step, (flat, sc, x) in enumerate(ran):
            osc, _, _ = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64))
            tol = dict(UNIFORM_TOLS)["sym"]
            print(f"[sym] {kernel} d={d} N={N} step {step}: sym {sc['sym']!r} oracle {osc['sym']!r} rel {abs(sc['sym'] - osc['sym']) / max(abs(osc['sym']), 1e-6):.2e}")
            assert osc["sym"] > 0 and abs(sc["sym"] - osc["sym"]) <= tol * max(abs(osc["sym"]), 1e-6), (kernel, d, N, step, sc["sym"], osc["sym"])
    eng.close()


# ---- 2. the full list is the plain / the graded sampler -------------------------------------------------------------------------------
@pytest.mark.parametrize("graded", [False, True], ids=["uniform", "graded"])
def test_the_full_list_is_the_sampler_it_indexes(graded):
    every = 3
    g = GRID[2]
    full = np.arange(120, dtype=np.int64)
    x_bc = _inputs(dict(layers=[2, 32, 32, 1]), 10)[2]
    engs = []
    for cells in (None, full):
        eng, _, _ = small_engine(2, dx=1.0 if graded else VOL[2], w_bc=10.0)
        eng.bind_boundary(dev(x_bc))
        if cells is None and graded:
            eng.bind_sampler_graded(EDGES[2], every=every, seed=SEED, draw0=1)
        elif cells is None:
            eng.bind_sampler(every=every, seed=SEED, draw0=1, **g)
        else:
            eng.bind_sampler_cells(cells, every=every, seed=SEED, draw0=1, edges=EDGES[2] if graded else None, **g)
        engs.append(eng)
    a, b = engs
    assert a.active_kernels == b.active_kernels
    assert same(a.sampler_points()[0], b.sampler_points()[0])
    if graded:
        wa, wb = a.weights(), b.weights()
        assert same(wa["q"], wb["q"])
        # W is formed differently: the graded sampler multiplies the per-axis fp64 sums of the fp32 widths, the list adds the fp32 cell
        # volumes, each of which carries the rounding of one fp32 multiply in 2D (2^-24 relative): the two agree to that, not bit for bit
        assert abs(wa["total"] - wb["total"]) <= 2.0 ** -24 * wa["total"]
        # Why the bits below survive a differing W: in this configuration (Rayleigh lambda, no regulariser) the reverse pass reads W through
        # one fp32 factor, float(2 w_pde / W) of the seeds, and for THESE edges the two totals -- 7e-9 apart, a quarter of an fp32 half-ulp --
        # round to the same fp32 factors; the fp64 loss does differ in its last digits, and under SCHED_CONST no step reads it.  This is
        # a fact of these edges, fixed by the inputs, not a law: test_the_full_graded_list_trains_as_the_graded_sampler_at_the_same_W
        # below is the statement that holds for any edges.
        assert np.float32(2.0 / wa["total"]) == np.float32(2.0 / wb["total"])          # (w_pde = 1: the factor itself)
    for e in engs:
        e.run(3 * every)
    assert a.sampler_points()[1] == b.sampler_points()[1] == 1 + 2
    assert same(a.sampler_points()[0], b.sampler_points()[0])
    assert same(a.get_grad(), b.get_grad()) and same_state(state(a), state(b))
    a.close(); b.close()


def test_the_full_graded_list_trains_as_the_graded_sampler_at_the_same_W():
    """the graded sampler's W is a product of per-axis fp64 sums, the list's a sum over the cells: the two differ in the last bits, and the
    step divides by W.  An engine on bind_points + bind_weights with the LIST's W per chunk of `every` steps is the plain machinery the
    graded sampler is held to (tests/test_gpu_weights.py), and the cell sampler equals it bit for bit."""
    every, steps = 3, 9
    full = np.arange(120, dtype=np.int64)
    a, _, _ = small_engine(2)
    a.bind_sampler_cells(full, every=every, seed=SEED, edges=EDGES[2], **GRID[2])
    a.run(steps)
    b, _, _ = small_engine(2)
    for m in range(steps // every):
        b.bind_points(dev(S.graded_points(EDGES[2], SEED, m)))
        b.bind_weights(dev(S.graded_weights(EDGES[2])), total=S.cells_total(full, EDGES[2]))
        b.run(every)
    assert same(a.get_grad(), b.get_grad()) and same_state(state(a), state(b))
    a.close(); b.close()


# ---- 3. rows of a block ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graded", [False, True], ids=["uniform", "graded"])
def test_a_block_of_rows_holds_its_rows_of_the_world_1_set(graded):
    first, n, every = 17, 23, 2
    eng, _, _ = small_engine(2)
    eng.bind_sampler_cells(DISK, every=every, seed=SEED, edges=EDGES[2] if graded else None, first=first, n_local=n, **GRID[2])
    assert eng.n_local == n
    for steps, draw in ((0, 0), (every + 1, 1)):
        if steps:
            eng.run(steps)
        pts, got = eng.sampler_points()
        assert got == draw and tuple(pts.shape) == (n, 2)
        assert same(pts, want_points(2, graded, draw)[first:first + n])
    cells, f = eng.sampler_cells()
    assert f == first and np.array_equal(cells, DISK)          # the engine holds the whole list, and rows 17 .. 39 of it
    if graded:
        w = eng.weights()
        q = S.cells_weights(DISK, EDGES[2])
        assert same(w["q"], q[first:first + n]) and w["total"] == S.cells_total(DISK, EDGES[2])
        assert abs(w["local"] - q[first:first + n].sum(dtype=np.float64)) <= 1e-12 * w["total"]
    eng.close()


# ---- 4. one step behind a redraw against the fp64 oracle ------------------------------------------------------------------------------
def _report(tag, sc, osc, keys, grad, ograd, layers):
    errs = H.block_rel_errs(grad, ograd, H.param_blocks(layers))
    print(tag, {k: (sc[k], osc[k]) for k, _ in keys if k in osc and k in sc}, "gradient rel err", H.rel_err(grad, ograd), "per block", errs)


@pytest.mark.parametrize("graded", [False, True], ids=["uniform", "graded"])
def test_real_psi_step_behind_a_redraw_matches_the_oracle(graded):
    kw = dict(layers=[2, 32, 32, 1], gamma=50.0, dx=1.0 if graded else VOL[2])
    _, flat, x_bc = _inputs(kw, 10)
    pb = go.Problem(**kw)
    eng = Engine(cfg_from_problem(pb, sched=capi.SCHED_CONST))
    eng.set_params(flat)
    eng.bind_boundary(dev(x_bc))
    eng.bind_sampler_cells(DISK, every=1, seed=SEED, edges=EDGES[2] if graded else None, **GRID[2])
    eng.step()
    flat1 = eng.get_params()
    sc = eng.step()                                   # redraws to draw 1, then steps on it
    pts, draw = eng.sampler_points()
    assert draw == 1 and same(pts, want_points(2, graded, 1))
    x64 = pts.cpu().numpy().astype(np.float64)
    grad = eng.get_grad()
    if graded:
        w = eng.weights()
        osc, ograd, _ = weighted_loss_and_grad(pb, flat1, pts.cpu().numpy(), w["q"].cpu().numpy(), x_bc.astype(np.float64), W=w["total"])
        _report("graded", sc, osc, UNIFORM_TOLS, grad, ograd, pb.layers)
        check_scalars(sc, osc)
    else:
        osc, ograd, _ = go.full_loss_and_grad(pb, flat1.astype(np.float64), x64, x_bc.astype(np.float64))
        _report("uniform", sc, osc, UNIFORM_TOLS, grad, ograd, pb.layers)
        for k, tol in UNIFORM_TOLS:
            assert abs(sc[k] - osc[k]) <= tol * max(abs(osc[k]), 1e-6), (k, sc[k], osc[k])
    assert H.rel_err(grad, ograd) < 5e-5
    bad = H.block_failures(grad, ograd, pb.layers)
    assert not bad, bad
    eng.close()


@pytest.mark.parametrize("graded", [False, True], ids=["uniform", "graded"])
def test_mixture_step_behind_a_redraw_matches_the_reference(graded):
    layers, cells = [1, 32, 32, 2], LIST[1]
    mp = mc.problem(layers, cells.size, dx=1.0 if graded else VOL[1])
    _, flat, x_bc, tgt = mc.inputs(layers, cells.size)
    eng = Engine(mix_config(mp, sched=capi.SCHED_CONST))
    try:
        eng.set_params(flat)
        eng.bind_boundary(dev(x_bc), dev(tgt))
        eng.bind_sampler_cells(cells, every=1, seed=SEED, edges=EDGES[1] if graded else None, **GRID[1])
        eng.step()
        flat1 = eng.get_params()
        got = mix_record(eng, eng.step())
        pts, draw = eng.sampler_points()
        assert draw == 1 and same(pts, want_points(1, graded, 1))
        q, W = (None, None)
        if graded:
            w = eng.weights()
            q, W = w["q"].cpu().numpy().astype(np.float64), w["total"]
            assert W == S.cells_total(cells, EDGES[1])
        sc, ograd, _ = mr.loss_and_grad(mp, flat1.astype(np.float64), pts.cpu().numpy().astype(np.float64), x_bc.astype(np.float64),
                                        tgt.astype(np.float64), q=q, W=W)
        grad = eng.get_grad()
        print("mixture", graded, {k: (got[k], sc[k]) for k in ("mu1", "mu2", "loss", "pde", "bc", "norm")}, "gradient rel err", H.rel_err(grad, ograd))
        bad = mix_failures(got, grad, sc, ograd, layers)
        assert not bad, bad
    finally:
        eng.close()


# ---- 5. graph replay ----------------------------------------------------------------------------------------------------------------
def test_graph_replay_changes_nothing():
    """52 points, every = 5, run(23): the replays are cut at every redraw.  GPE_GRAPH is read at gpe_create."""
    assert DISK.size <= 64
    out = []
    for graph in ("1", "0"):
        with environment({"GPE_GRAPH": graph}):
            eng, _, _ = small_engine(2, dx=VOL[2])
        eng.bind_sampler_cells(DISK, every=5, seed=SEED, **GRID[2])
        eng.run(23)
        pts, draw = eng.sampler_points()
        assert draw == 22 // 5 and same(pts, want_points(2, False, draw))
        out.append(state(eng))
        eng.close()
    assert out[0][3] == 23 and same_state(out[0], out[1])


# ---- 6. three ranks by hand ---------------------------------------------------------------------------------------------------------
def test_three_ranks_by_hand_match_the_weighted_reference_on_all_points():
    K = DISK.size
    kw = dict(layers=[2, 32, 32, 1], gamma=50.0, dx=1.0)
    _, flat, x_bc = _inputs(kw, 10)
    pb = go.Problem(**kw)
    cuts = H.dp_cuts(3, K)
    assert [hi - lo for lo, hi in cuts] == [1, 17, K - 18]
    W = S.cells_total(DISK, EDGES[2])
    x, q = want_points(2, True, 0), S.cells_weights(DISK, EDGES[2])
    osc, ograd, _ = weighted_loss_and_grad(pb, flat, x, q, x_bc.astype(np.float64), W=W)
    engs = []
    try:
        for lo, hi in cuts:
            e = Engine(cfg_from_problem(pb, world_size=3))
            engs.append(e)
            e.set_params(flat)
            e.bind_boundary(dev(x_bc))
            e.bind_sampler_cells(DISK, every=10, seed=SEED, edges=EDGES[2], first=lo, n_local=hi - lo, **GRID[2])
            w = e.weights()
            assert w["total"] == W and same(e.sampler_points()[0], x[lo:hi]) and same(w["q"], q[lo:hi])
        dp_step(engs)
        scs = [e.read_scalars() for e in engs]
        grad = engs[0].get_grad()
        _report("dp", scs[0], osc, UNIFORM_TOLS, grad, ograd, pb.layers)
        check_scalars(scs[0], osc)
        assert H.rel_err(grad, ograd) < 5e-5
        p0 = engs[0].get_params()
        for r in (1, 2):
            assert scs[r]["loss"] == scs[0]["loss"] and scs[r]["mu"] == scs[0]["mu"]
            assert same(engs[r].get_params(), p0)
    finally:
        for e in engs:
            e.close()


# ---- 7. frozen orthogonality state ---------------------------------------------------------------------------------------------------
def test_frozen_orthogonality_state_is_refilled_behind_a_redraw():
    kw = dict(layers=[2, 32, 32, 1], gamma=20.0, dx=VOL[2], w_bc=0.0, w_orth=2.0)
    eng, _, _ = small_engine(2, dx=VOL[2], w_orth=2.0)
    theta = _frozen(kw, 1)
    eng.bind_orth_state(0, theta)
    eng.bind_sampler_cells(DISK, every=1, seed=SEED, **GRID[2])
    psi0 = eng.orth_values(0).cpu().numpy()
    assert close(psi0, _oracle_psi(kw, theta, want_points(2, False, 0)), 5e-6, 2e-6)
    eng.step(); eng.step()
    pts, draw = eng.sampler_points()
    psi1 = eng.orth_values(0).cpu().numpy()
    assert draw == 1 and psi1.shape == (DISK.size,) and not np.array_equal(psi0, psi1)
    assert close(psi1, _oracle_psi(kw, theta, pts.cpu().numpy()), 5e-6, 2e-6)
    eng.close()


# ---- 8. symmetry batch ---------------------------------------------------------------------------------------------------------------
def test_the_symmetry_batch_follows_the_redraw():
    kw = dict(CASES["1d_32x4_nb_sym"][0], dx=VOL[1])
    assert kw["w_sym"] != 0
    _, flat, x_bc = _inputs(kw, 10)
    pb = go.Problem(**kw)
    eng = Engine(cfg_from_problem(pb, sched=capi.SCHED_CONST))
    eng.set_params(flat)
    eng.bind_boundary(dev(x_bc))
    eng.bind_sampler_cells(LIST[1], every=1, seed=SEED, **GRID[1])
    eng.step()
    flat1 = eng.get_params()
    sc = eng.step()                                   # [x ; -x] of draw 1: a batch left on draw 0 would miss the sym term
    pts, draw = eng.sampler_points()
    assert draw == 1 and same(pts, want_points(1, False, 1))
    x64 = pts.cpu().numpy().astype(np.float64)
    osc, ograd, _ = go.full_loss_and_grad(pb, flat1.astype(np.float64), x64, x_bc.astype(np.float64))
    stale, _, _ = go.full_loss_and_grad(pb, flat1.astype(np.float64), want_points(1, False, 0).astype(np.float64), x_bc.astype(np.float64))
    grad = eng.get_grad()
    _report("sym", sc, osc, UNIFORM_TOLS, grad, ograd, pb.layers)
    assert osc["sym"] > 0 and abs(stale["sym"] - osc["sym"]) > 10 * 1e-4 * osc["sym"]          # (the two draws are told apart: 10 x the bound)
    for k, tol in UNIFORM_TOLS:
        assert abs(sc[k] - osc[k]) <= tol * max(abs(osc[k]), 1e-6), (k, sc[k], osc[k])
    assert H.rel_err(grad, ograd) < 5e-5
    # the graded form has no symmetry batch: refused as the graded sampler refuses it, the uniform sampler stays
    assert code(eng.bind_sampler_cells, LIST[1], every=1, seed=SEED, edges=EDGES[1], **GRID[1]) == capi.GPE_ERR_INVALID
    assert eng.sampler_points()[1] == 1
    eng.close()


# ---- 9. replacing and clearing ----------------------------------------------------------------------------------------------------
def test_replacing_and_clearing():
    g = GRID[2]
    binds = [("plain", lambda e: e.bind_sampler(every=3, seed=5, **g), lambda: S.stratified_points(seed=5, draw=0, **g), None),
             ("cells", lambda e: e.bind_sampler_cells(DISK, every=3, seed=6, **g), lambda: S.cells_points(DISK, seed=6, draw=0, **g), None),
             ("graded", lambda e: e.bind_sampler_graded(EDGES[2], every=3, seed=7), lambda: S.graded_points(EDGES[2], 7, 0),
              lambda: (S.graded_weights(EDGES[2]), S.graded_total(EDGES[2]))),
             ("graded cells", lambda e: e.bind_sampler_cells(DISK, every=3, seed=8, edges=EDGES[2], **g),
              lambda: S.cells_points(DISK, seed=8, draw=0, edges=EDGES[2], **g),
              lambda: (S.cells_weights(DISK, EDGES[2]), S.cells_total(DISK, EDGES[2]))),
             ("cells again", lambda e: e.bind_sampler_cells(DISK[3:], every=3, seed=9, **g), lambda: S.cells_points(DISK[3:], seed=9, draw=0, **g), None)]
    eng, _, flat = small_engine(2)
    for name, bind, points, weights in binds:
        bind(eng)
        eng.step()                                    # (a step on every sampler, so each bind replaces a used one)
        fresh, _, _ = small_engine(2)
        bind(fresh)
        bind(eng)
        pts, draw = eng.sampler_points()
        assert draw == 0 and same(pts, points()), name
        assert eng.active_kernels == fresh.active_kernels, name
        if weights is None:
            assert code(eng.weights) == capi.GPE_ERR_STATE, name
        else:
            w = eng.weights()
            assert same(w["q"], weights()[0]) and w["total"] == weights()[1], name
        if "cells" in name:
            assert eng.sampler_cells()[0].size == (DISK.size - 3 if "again" in name else DISK.size)
        else:
            assert code(eng.sampler_cells) == capi.GPE_ERR_STATE, name
        fresh.close()
    # the caller's points take over: list, weights and sampler go, and the step is the step of an engine that never had a sampler
    x = np.random.default_rng(2).uniform(-2, 2, (77, 2)).astype(np.float32)
    eng.set_params(flat)
    eng.reset_optimizer(1e-3)
    eng.bind_points(dev(x))
    for fn in (eng.sampler_points, eng.sampler_cells, eng.weights):
        assert code(fn) == capi.GPE_ERR_STATE
    fresh, _, _ = small_engine(2)
    fresh.bind_points(dev(x))
    assert eng.active_kernels == fresh.active_kernels
    sa, sb = eng.step(), fresh.step()
    assert all(sa[k] == sb[k] for k in ("loss", "mu", "pde", "norm", "grad_norm")), (sa, sb)
    assert same(eng.get_grad(), fresh.get_grad()) and same(eng.get_params(), fresh.get_params())
    # clear_sampler clears a cell sampler as any other
    eng.bind_sampler_cells(DISK, every=3, seed=6, edges=EDGES[2], **g)
    eng.clear_sampler()
    for fn in (eng.sampler_points, eng.sampler_cells, eng.weights, eng.step):
        assert code(fn) == capi.GPE_ERR_STATE
    eng.close(); fresh.close()


# ---- 10. refusals, each leaving the engine as it was -----------------------------------------------------------------------------------
def _raw(eng, cells, n_cells=None, edges=(None, None, None), **spec):
    """gpe_sampler_cells through ctypes, for what the Python helper would refuse first: -> (code, message)"""
    g = dict(GRID[2], every=3, first=0, n_local=None)
    g.update(spec)
    sp = capi.gpe_sampler_spec()
    for k in range(len(g["shape"])):
        sp.shape[k], sp.lo[k], sp.hi[k], sp.clip_lo[k], sp.clip_hi[k] = g["shape"][k], g["lo"][k], g["hi"][k], g["lo"][k], g["hi"][k]
    c = None if cells is None else np.ascontiguousarray(cells, dtype=np.int64)
    n_cells = (0 if c is None else c.size) if n_cells is None else n_cells
    sp.first_cell, sp.n_local = g["first"], n_cells - g["first"] if g["n_local"] is None else g["n_local"]
    sp.seed, sp.every = SEED, g["every"]
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = eng.lib.gpe_sampler_cells(eng._h, C.byref(sp), ptr(c), n_cells, *[ptr(e) for e in edges])
    return rc, (eng.lib.gpe_last_error(eng._h) or b"").decode()


def _refusals():
    e0, e1 = EDGES[2]
    flat_edge = e0.copy(); flat_edge[3] = flat_edge[2]
    nan_edge = e0.copy(); nan_edge[2] = np.nan
    return {
        "no list": (dict(cells=None, n_cells=5), "n_cells"),
        "empty list": (dict(cells=DISK, n_cells=0), "n_cells"),
        "negative count": (dict(cells=DISK, n_cells=-3), "n_cells"),
        "not ascending": (dict(cells=[0, 5, 5, 9]), "position 2"),
        "descending": (dict(cells=[0, 5, 9, 8, 7]), "position 3"),
        "cell beyond the grid": (dict(cells=[0, 5, 120]), "cells[2] = 120"),
        "negative cell": (dict(cells=[-1, 5]), "cells[0] = -1"),
        "first < 0": (dict(cells=DISK, first=-1, n_local=5), "rows"),
        "n_local = 0": (dict(cells=DISK, n_local=0), "rows"),
        "rows beyond the list": (dict(cells=DISK, first=DISK.size - 2, n_local=3), "rows"),
        "rows beyond the list, within the grid": (dict(cells=DISK, first=0, n_local=DISK.size + 1), "rows"),
        "every = 0": (dict(cells=DISK, every=0), "every"),
        "every < 0": (dict(cells=DISK, every=-2), "every"),
        "hi <= lo": (dict(cells=DISK, hi=(3.0, -2.5)), "hi <= lo"),
        "one axis for two": (dict(cells=[0, 1], shape=(120,), lo=(-3.0,), hi=(3.0,)), "input axes"),
        "three axes for two": (dict(cells=[0, 1], shape=(12, 5, 2), lo=(-3.0, -2.5, -1.0), hi=(3.0, 2.5, 1.0)), "input axes"),
        "axis index beyond 2^24": (dict(cells=[0, 1], shape=(2 ** 24 + 1, 10)), "2^24"),
        "edges for one axis of two": (dict(cells=DISK, edges=(e0, None, None)), "no edges for axis 1"),
        "edges for the other axis": (dict(cells=DISK, edges=(None, e1, None)), "no edges for axis 0"),
        "edges that do not increase": (dict(cells=DISK, edges=(flat_edge, e1, None)), "do not increase"),
        "an edge that is not finite": (dict(cells=DISK, edges=(nan_edge, e1, None)), "not finite"),
        "lo other than the first edge": (dict(cells=DISK, edges=(e0, e1, None), lo=(-2.5, -2.5)), "first / last edge"),
    }


@pytest.mark.parametrize("bound", ["points", "cell sampler"])
def test_refused_binds_leave_the_engine_as_it_was(bound):
    """an engine that meets every refusal between its steps against a twin that meets none: the same bits throughout"""
    x = dev(np.random.default_rng(0).uniform(-3, 3, (400, 2)))
    pair = []
    for _ in range(2):
        eng, _, _ = small_engine(2)
        if bound == "points":
            eng.bind_points(x)
        else:
            eng.bind_sampler_cells(DISK, every=2, seed=SEED, edges=EDGES[2], **GRID[2])
        pair.append(eng)
    a, twin = pair
    for name, (args, text) in _refusals().items():
        rc, msg = _raw(a, **args)
        assert rc == capi.GPE_ERR_INVALID and msg.startswith("sampler_cells:") and text in msg, (name, rc, msg)
        if bound == "points":
            assert code(a.sampler_points) == capi.GPE_ERR_STATE and code(a.sampler_cells) == capi.GPE_ERR_STATE, name
        else:
            assert a.weights()["total"] == twin.weights()["total"], name
        sa, st = a.step(), twin.step()
        assert sa == st and same(a.get_params(), twin.get_params()), name
    if bound == "cell sampler":
        assert a.sampler_points()[1] == twin.sampler_points()[1] > 3 and same(a.sampler_points()[0], twin.sampler_points()[0])
    # an array on fixed points: refused, and fine again once it is gone
    a.bind_orth(0, None)
    if bound == "points":
        a.bind_orth(0, torch.ones(400, device="cuda"))
        rc, msg = _raw(a, DISK)
        assert rc == capi.GPE_ERR_INVALID and "orthogonality array 0" in msg
        a.bind_orth(0, None)
    rc, msg = _raw(a, DISK)
    assert rc == capi.GPE_OK, msg
    assert np.array_equal(a.sampler_cells()[0], DISK)
    a.close(); twin.close()


def test_problems_that_live_on_fixed_points_refuse_the_cell_sampler():
    x = dev(np.random.default_rng(0).uniform(-3, 3, (400, 2)))
    V = torch.zeros(400, device="cuda")
    pair = []
    for _ in range(2):
        eng, _, _ = small_engine(2, potential=capi.POT_PRECOMPUTED)
        eng.bind_points(x, V=V)
        pair.append(eng)
    a, twin = pair
    rc, msg = _raw(a, DISK)
    assert rc == capi.GPE_ERR_INVALID and "precomputed potential" in msg
    assert a.step() == twin.step() and same(a.get_params(), twin.get_params())
    a.close(); twin.close()
    base = Engine(cfg_from_problem(go.Problem(layers=[1, 32, 32, 1], gamma=1.0, dx=0.01, w_bc=0.0, base_mode=0, base_kind=capi.BASE_PRECOMPUTED)))
    assert code(base.bind_sampler_cells, LIST[1], every=5, **GRID[1]) == capi.GPE_ERR_INVALID
    base.close()


def test_arrays_on_fixed_points_and_lbfgs_are_refused_as_under_any_sampler():
    msgs = {}
    for kind in ("plain", "cells"):
        eng, _, _ = small_engine(1, dx=VOL[1])
        eng.lbfgs_config(0.1, history=3)
        if kind == "plain":
            eng.bind_sampler(every=2, seed=1, **GRID[1])
        else:
            eng.bind_sampler_cells(LIST[1], every=2, seed=1, **GRID[1])
        n = eng.n_local
        ones = torch.ones(n, device="cuda")
        got = []
        for call in (lambda: eng.lbfgs_run(1), eng.lbfgs_update, lambda: eng.bind_orth(0, ones), lambda: eng.bind_target(ones), eng.mse_step,
                     eng.mse_loss_grad, lambda: eng.bind_weights(ones)):
            with pytest.raises(GPEError) as ex:
                call()
            assert ex.value.code == capi.GPE_ERR_STATE
            got.append(str(ex.value))
        assert "sampler" in got[0] and "sampler" in got[1]
        msgs[kind] = got
        eng.step()                                    # still usable
        eng.close()
    assert msgs["plain"] == msgs["cells"]
