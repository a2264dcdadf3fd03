"""Analytic potential terms on the device (include/gpe_hip.h: gpe_potential_terms; csrc/gpe_potential.h), one small shape per kernel
family (tests.live_table.CLASSES).

  values      potential_at(x) against gpe_pinn.potential.evaluate(..., float64) within potential.error_bound, U = U_DEVICE: the error of
              expf / cosf themselves, measured by tools/potential_ulp.py over these very inputs (profiles/potential/values_ulp.txt),
              doubled and rounded up -- see tests/potential_cases.py for why it is not the error of the whole term
  same path   an engine with terms against a twin fed potential_values() as a caller's d_V: bit-identical after 5 steps
  oracle      first step's record and gradient against oracle.gpe_oracle with V_pre = evaluate(..., float64); the bounds of
              tests/test_gpu_parity.py: loss 1e-4, mu 2e-5, gradient 5e-5.  Not the mixture class: tests/test_gpu_parity.py has no bound
              for it, so a mixture step with terms is held by the twin comparison (same path) and the observers only
  harmonic    one QUAD term against a GPE_POT_HARMONIC engine
  redraws     every sampler on the grids of tests/test_sampler_plan.py -- (12, 10) in 2D: plain, graded, adaptive, cell subset, and a block
              (first_cell = 7, 50 rows: what one rank of step_dp holds) of the plain and the graded grid; (16,) in 1D and (6, 5, 4) in 3D:
              plain, graded and one more each -- every = 3, run(20): the held set against gpe_pinn.sampler, V of the held draw,
              GPE_GRAPH=0 against GPE_GRAPH=1 bit for bit (the replaying engine with GPE_GRAPH_STEPS=3: gpe_run never replays across a redraw,
              so 8-step graphs would never run here), and the record of step 20 against the oracle on the held set -- for the weighted
              samplers PC.weighted_loss_and_grad (the reference of tests/weighted_ref.py with V_pre per point) with the weights the engine
              holds.  tests/test_potential_terms_cpu.py shows a stale V cannot pass any of them
  live        the lattice depth x 3 between steps 8 and 9, replayed and not
  observers   observables(x_eval), the monitor and the keeper without V on a held-out set; the mixture variants once
  frozen      a frozen orthogonality state + the plain sampler + terms over one redraw
  refusals    each on a live engine that works afterwards
"""
import os

import numpy as np
import pytest

from gpe_pinn import Engine, GPEError, capi
from gpe_pinn import keeper as K
from gpe_pinn import potential as pot
from gpe_pinn import sampler as S
from oracle import gpe_oracle as go
from tests import helpers as H
from tests import live_table as T
from tests import potential_cases as PC
from tests.test_observables_cpu import observables_ref

pytestmark = pytest.mark.gpu

U_DEVICE = PC.U_DEVICE


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _ctx(cls, terms=None):
    """the class's start state on the precomputed-potential path; terms: V = the fp64 reference on the class's points"""
    ctx = T.start(cls)
    if ctx["mix"]:
        ctx["engine_kw"]["potential"] = go.POT_PRECOMPUTED
    else:
        ctx["kw"]["potential"] = go.POT_PRECOMPUTED
    if terms is not None:
        ctx["V"] = pot.evaluate(terms, ctx["x"], np.float64)
    return ctx


def _engine(ctx, terms, graph=None, env=None):
    env = dict(env or {})
    if graph is not None:
        env["GPE_GRAPH"] = graph
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine(T.config(ctx))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    eng.set_params(ctx["flat"])
    if terms is not None:
        eng.bind_potential_terms(terms)
    return eng


def _bind(eng, ctx, V=None):
    eng.bind_points(ctx["x"], V=V)
    if ctx["x_bc"] is not None:
        eng.bind_boundary(ctx["x_bc"], ctx["tgt"])


def _terms_for(cls):
    return PC.trap4(T.CLASSES[cls]["kw"]["layers"][0])


def _held_within_bound(got, terms, x):
    ref = pot.evaluate(terms, x, np.float64)
    bound = pot.error_bound(terms, x, U_DEVICE)
    err = np.abs(np.asarray(got, np.float64) - ref)
    i = int(np.argmax(err / np.maximum(bound, 1e-300)))
    print(f"   V: max |err| / bound = {err[i] / max(bound[i], 1e-300):.3f} at row {i} (err {err[i]:.3e}, bound {bound[i]:.3e})")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (i, got[i], ref[i], err[i], bound[i])


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------------
ROWS = (1, 63, 64, 65, 257)               # 257 = one workgroup of k_potential_terms plus one


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_values_meet_the_fp64_reference(dim):
    cls = {1: "coop", 2: "h128", 3: "wide"}[dim]
    eng = _engine(_ctx(cls), None)
    try:
        tables = {k: PC.single(k, dim) for k in PC.KINDS}
        tables["mix16"] = PC.mix16(dim)
        for name, terms in tables.items():
            eng.bind_potential_terms(terms)
            back = eng.potential_terms()
            assert len(back) == len(terms) and all(b.kind == t.kind and np.float32(b.a) == np.float32(t.a) for b, t in zip(back, terms))
            for n in ROWS:
                x = PC.points(dim, n, seed=n)
                got = eng.potential_at(x).cpu().numpy()
                print(f"{name} dim {dim} n {n}")
                _held_within_bound(got, terms, x)
    finally:
        eng.close()


# ---- 2. same path, 3. oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", T.ALL)
def test_terms_run_the_precomputed_path_bit_for_bit(cls):
    terms = _terms_for(cls)
    ctx = _ctx(cls, terms)
    a = b = None
    try:
        a, b = _engine(ctx, terms), _engine(ctx, None)
        _bind(a, ctx)
        V = a.potential_values()
        assert V.shape == (ctx["N"],)
        _held_within_bound(V.cpu().numpy(), terms, ctx["x"])
        _bind(b, ctx, V=V)
        assert a.active_kernels == b.active_kernels
        for _ in range(5):
            sa, sb = a.step(), b.step()
        assert sa == sb and sa["step"] == 5 and np.isfinite(sa["loss"])
        assert np.array_equal(_bits(a.get_params()), _bits(b.get_params())) and np.array_equal(_bits(a.get_grad()), _bits(b.get_grad()))
    finally:
        for e in (a, b):
            if e is not None:
                e.close()


def _check_step(sc, grad, ctx, flat=None):
    pb = T.problem(ctx)
    f64 = lambda v: None if v is None else np.asarray(v, np.float64)
    osc, ograd, _ = go.full_loss_and_grad(pb, f64(ctx["flat"] if flat is None else flat), f64(ctx["x"]), f64(ctx["x_bc"]), f64(ctx["tgt"]), f64(ctx["V"]),
                                          T.orth_rows(ctx))
    print(f"   loss {sc['loss']:.9g} (oracle {osc['loss']:.9g}, rel {abs(sc['loss'] - osc['loss']) / abs(osc['loss']):.2e})  "
          f"mu {sc['mu']:.9g} (oracle {osc['mu']:.9g}, rel {abs(sc['mu'] - osc['mu']) / abs(osc['mu']):.2e})")
    assert abs(sc["loss"] - osc["loss"]) <= 1e-4 * abs(osc["loss"]), (sc["loss"], osc["loss"])
    assert abs(sc["mu"] - osc["mu"]) <= 2e-5 * abs(osc["mu"]), (sc["mu"], osc["mu"])
    if grad is not None:
        assert H.rel_err(grad, ograd) < 5e-5


@pytest.mark.parametrize("cls", T.NONMIX)
def test_first_step_meets_the_oracle(cls):
    terms = _terms_for(cls)
    ctx = _ctx(cls, terms)
    eng = _engine(ctx, terms)
    try:
        _bind(eng, ctx)
        sc = eng.step()
        _check_step(sc, eng.get_grad(), ctx)
    finally:
        eng.close()


# ---- 4. harmonic equivalence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["coop", "h128", "wide"])
def test_one_quad_term_is_the_harmonic_engine(cls):
    ctx0 = T.start(cls)                                   # (these classes are harmonic: pot_scale, omega from the class)
    pb = T.problem(ctx0)
    d = pb.layers[0]
    ctx0["kw"]["pot_a"] = 0.35                            # an off-centre trap along x
    term = [pot.quadratic(pb.pot_scale, tuple(pb.omega[:d]), (0.35,) + (0.0,) * (d - 1))]
    ctx1 = _ctx(cls, term)
    a = b = None
    try:
        a, b = _engine(ctx0, None), _engine(ctx1, term)
        _bind(a, ctx0); _bind(b, ctx1)
        V = b.potential_values().cpu().numpy()
        assert np.array_equal(_bits(V), _bits(pot.evaluate(term, ctx1["x"], np.float32)))      # pot_scale * sum (omega (x - c))^2, in fp32 with fmaf
        sa, sb = a.step(), b.step()
        _check_step(sa, a.get_grad(), ctx0)
        _check_step(sb, b.get_grad(), ctx1)
    finally:
        for e in (a, b):
            if e is not None:
                e.close()


# ---- 5. redraws ---------------------------------------------------------------------------------------------------------------------------
# the grids of tests/test_sampler_plan.py: (16,) in 1D, (12, 10) in 2D, (6, 5, 4) in 3D, their sinh edges, block edges and cell lists
from tests.test_sampler_plan import BLOCKS as PLAN_BLOCKS, EDGES as PLAN_EDGES, GRID as PLAN_GRID, LIST as PLAN_LIST      # noqa: E402

GRID, EDGES, BLOCKS, DISK = PLAN_GRID[2], PLAN_EDGES[2], PLAN_BLOCKS[2], PLAN_LIST[2]
SEED, EVERY = PC.SAMPLER_SEED, 3
DIM_CLASS = {1: "coop", 2: "h128", 3: "wide"}
BLOCK = (7, 50)                                       # a block of the 2D grid: first_cell, n_local (what one rank of step_dp holds)
AD_POINTS = {1: 40, 2: 96, 3: 60}
REDRAW_CASES = [(2, "plain"), (2, "graded"), (2, "adaptive"), (2, "cells"), (2, "block"), (2, "graded_block"),
                (1, "plain"), (1, "graded"), (1, "adaptive"), (3, "plain"), (3, "graded"), (3, "cells")]


def _bind_sampler(eng, kind, dim=2):
    g = PLAN_GRID[dim]
    if kind == "plain":
        eng.bind_sampler(g["lo"], g["hi"], g["shape"], every=EVERY, seed=SEED)
    elif kind == "block":
        eng.bind_sampler(g["lo"], g["hi"], g["shape"], every=EVERY, seed=SEED, first_cell=BLOCK[0], n=BLOCK[1])
    elif kind == "graded":
        eng.bind_sampler_graded(PLAN_EDGES[dim], every=EVERY, seed=SEED)
    elif kind == "graded_block":
        eng.bind_sampler_graded(PLAN_EDGES[dim], every=EVERY, seed=SEED, first_cell=BLOCK[0], n=BLOCK[1])
    elif kind == "adaptive":
        eng.bind_sampler_adaptive(PLAN_BLOCKS[dim], n_points=AD_POINTS[dim], every=EVERY, seed=SEED, n_min=2)
    else:
        eng.bind_sampler_cells(PLAN_LIST[dim], g["lo"], g["hi"], g["shape"], every=EVERY, seed=SEED)


def _sampler_ctx(kind, dim=2):
    ctx = _ctx(DIM_CLASS[dim])
    ctx["x_bc"] = None
    if kind == "cells":
        ctx["kw"]["n_global"] = int(PLAN_LIST[dim].size)
    return ctx


def _expected_points(kind, dim, draw):
    g = PLAN_GRID[dim]
    if kind == "plain":
        return S.stratified_points(g["lo"], g["hi"], g["shape"], SEED, draw)
    if kind == "block":
        return S.stratified_points(g["lo"], g["hi"], g["shape"], SEED, draw, first_cell=BLOCK[0], n=BLOCK[1])
    if kind == "graded":
        return S.graded_points(PLAN_EDGES[dim], SEED, draw)
    if kind == "graded_block":
        return S.graded_points(PLAN_EDGES[dim], SEED, draw, first_cell=BLOCK[0], n=BLOCK[1])
    if kind == "cells":
        return S.cells_points(PLAN_LIST[dim], g["lo"], g["hi"], g["shape"], SEED, draw)
    return None                                       # adaptive: the counts follow the residual; the points are read from the engine


@pytest.mark.parametrize("dim,kind", REDRAW_CASES)
def test_redraws_refill_the_potential(dim, kind):
    terms = PC.redraw_table(dim)
    ctx = _sampler_ctx(kind, dim)
    weighted = kind in ("graded", "graded_block", "adaptive")
    a = b = None
    try:
        a, b = _engine(ctx, terms, graph="1", env={"GPE_GRAPH_STEPS": "3"}), _engine(ctx, terms, graph="0")
        for e in (a, b):
            _bind_sampler(e, kind, dim)
        a.run(20)
        b.run(19)
        th19 = b.get_params()
        b.run(1)
        a.synchronize(); b.synchronize()
        assert np.array_equal(_bits(a.get_params()), _bits(b.get_params()))
        for e in (a, b):
            x, draw = e.sampler_points()
            assert draw == 6
            x = x.cpu().numpy()
            want = _expected_points(kind, dim, 6)
            assert x.shape[1] == dim and (want is None or np.array_equal(x, want))
            print(f"{kind} {dim}d: V of draw {draw} on {x.shape[0]} rows")
            _held_within_bound(e.potential_values().cpu().numpy(), terms, x)
        # the record of step 20 against the oracle on the held set, at the parameters step 19 left
        x = a.sampler_points()[0].cpu().numpy()
        V = pot.evaluate(terms, x, np.float64)
        rec = a.read_history(20, 1)[0]
        assert rec["step"] == 20
        if weighted:                                  # the held weights and W as the engine reports them (tests/test_gpu_weights.py reads them so)
            w = a.weights()
            q = w["q"].cpu().numpy()
            if kind == "graded":
                assert np.array_equal(q, S.graded_weights(PLAN_EDGES[dim])) and w["total"] == S.graded_total(PLAN_EDGES[dim])
            osc, _ = PC.weighted_loss_and_grad(T.problem(ctx), th19, x, q, V, W=w["total"])
            print(f"   loss {rec['loss']:.9g} (oracle {osc['loss']:.9g})  mu {rec['mu']:.9g} (oracle {osc['mu']:.9g})")
            assert abs(rec["loss"] - osc["loss"]) <= 1e-4 * abs(osc["loss"]), (rec["loss"], osc["loss"])
            assert abs(rec["mu"] - osc["mu"]) <= 2e-5 * abs(osc["mu"]), (rec["mu"], osc["mu"])
        else:
            _check_step(rec, None, dict(ctx, x=x, V=V), flat=th19)
    finally:
        for e in (a, b):
            if e is not None:
                e.close()


# ---- 6. live change -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["coop", "h128"])
def test_a_change_of_the_terms_shows_in_the_next_step_replayed_or_not(cls):
    terms, new = PC.live_tables(T.CLASSES[cls]["kw"]["layers"][0])
    ctx = _ctx(cls, terms)
    a = b = None
    try:
        a, b = _engine(ctx, terms, graph="1"), _engine(ctx, terms, graph="0")
        for e in (a, b):
            _bind(e, ctx)
            e.run(8)
        a.synchronize(); b.synchronize()
        th8 = a.get_params()
        assert np.array_equal(_bits(th8), _bits(b.get_params()))
        for e in (a, b):
            e.bind_potential_terms(new)
            e.run(8)
        a.synchronize(); b.synchronize()
        c2 = dict(ctx, V=pot.evaluate(new, ctx["x"], np.float64))
        for e in (a, b):
            rec = e.read_history(9, 1)[0]
            assert rec["step"] == 9
            _check_step(rec, None, c2, flat=th8)
            _held_within_bound(e.potential_values().cpu().numpy(), new, ctx["x"])
        assert np.array_equal(_bits(a.get_params()), _bits(b.get_params()))
    finally:
        for e in (a, b):
            if e is not None:
                e.close()


# ---- 7. monitor, observables, keeper -------------------------------------------------------------------------------------------------------
def _obs_ref(ctx, flat, x_eval, terms):
    from tests.test_gpu_observables import oracle_jets
    pb = T.problem(ctx)
    x64 = np.asarray(x_eval, np.float32).astype(np.float64)
    V = pot.evaluate(terms, x_eval, np.float64)
    return observables_ref(pb, x64, go.head_pde(pb, x64, oracle_jets(pb, np.asarray(flat), x64), V_pre=V), pb.dx)[0]


def test_observers_work_without_a_potential_array():
    terms = PC.trap4(2)
    ctx = _ctx("h128", terms)
    x_eval = PC.points(2, 257, seed=77, half=3.0)
    eng = _engine(ctx, terms)
    try:
        _bind(eng, ctx)
        got = eng.observables(x_eval)
        ref = _obs_ref(ctx, ctx["flat"], x_eval, terms)
        for k, tol in (("pot", 1e-4), ("mu", 2e-5)):                      # the tolerances of tests/test_gpu_observables.py: PARTS, TIGHT
            print(f"   {k}: {got[k]:.9g} ref {ref[k]:.9g}")
            assert abs(got[k] - ref[k]) <= tol * max(abs(ref[k]), 1e-6), (k, got[k], ref[k])
        eng.bind_monitor(x_eval, every=2)
        eng.bind_keeper("res_rms")
        eng.run(8)
        recs = eng.read_monitor()
        assert len(recs) == 4
        look = eng.observables(x_eval)                                   # stop and look: the same chain on the same parameters
        assert look == recs[-1]
        ref = _obs_ref(ctx, eng.get_params(), x_eval, terms)
        for k, tol in (("pot", 1e-4), ("mu", 2e-5)):
            assert abs(recs[-1][k] - ref[k]) <= tol * max(abs(ref[k]), 1e-6), (k, recs[-1][k], ref[k])
        kept = K.select([r["res_rms"] for r in recs])[0]
        assert eng.best_record() == recs[kept]
        # the monitor's V follows a change of the terms
        deeper = terms[:3] + [terms[3]._replace(a=3.0 * terms[3].a)]
        eng.bind_potential_terms(deeper)
        eng.run(2)
        last = eng.read_monitor()[-1]
        ref = _obs_ref(ctx, eng.get_params(), x_eval, deeper)
        assert abs(last["pot"] - ref["pot"]) <= 1e-4 * abs(ref["pot"]), (last["pot"], ref["pot"])
        with pytest.raises(GPEError) as ei:
            eng.clear_potential_terms()
        assert ei.value.code == capi.GPE_ERR_STATE and "monitor" in str(ei.value)
    finally:
        eng.close()


def test_mixture_observers_work_without_a_potential_array():
    terms = PC.trap4(2)
    ctx = _ctx("mix", terms)
    x_eval = PC.points(2, 65, seed=78, half=3.0)
    a = b = None
    try:
        a, b = _engine(ctx, terms), _engine(ctx, None)
        _bind(a, ctx)
        _bind(b, ctx, V=a.potential_values())
        Ve = a.potential_at(x_eval)
        _held_within_bound(Ve.cpu().numpy(), terms, x_eval)
        assert a.mixture_observables(x_eval) == b.mixture_observables(x_eval, V=Ve)
        a.bind_mixture_monitor(x_eval, every=2); b.bind_mixture_monitor(x_eval, every=2, V=Ve)
        a.run(4); b.run(4)
        ra, rb = a.read_mixture_monitor(), b.read_mixture_monitor()
        assert len(ra) == 2 and ra == rb and ra[0]["pot"][0] != 0.0
    finally:
        for e in (a, b):
            if e is not None:
                e.close()


# ---- 8. frozen state ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_frozen_state_and_terms_behind_a_redraw(dim):
    terms = PC.redraw_table(dim)
    ctx = _sampler_ctx("plain", dim)
    ctx["kw"]["w_orth"] = 5.0
    st = T._state_of(ctx, 2.0)
    eng = _engine(ctx, terms)
    try:
        T.bind_state(eng, st)
        _bind_sampler(eng, "plain", dim)
        eng.run(EVERY)                                                   # draw 0
        th = eng.get_params()
        rec = eng.step()                                                 # the step behind the redraw: draw 1
        x, draw = eng.sampler_points()
        assert draw == 1 and rec["step"] == EVERY + 1
        x = x.cpu().numpy()
        c2 = dict(ctx, x=x, V=pot.evaluate(terms, x, np.float64), orth_state=st)
        assert rec["orth"] > 0
        _check_step(rec, eng.get_grad(), c2, flat=th)
    finally:
        eng.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_working_engine():
    terms = PC.trap4(2)
    ctx = _ctx("h128", terms)
    eng = _engine(ctx, None)
    plain = Engine(T.config(T.start("h128")))
    try:
        with pytest.raises(GPEError) as ei:                              # terms on a non-precomputed config
            plain.bind_potential_terms(terms)
        assert ei.value.code == capi.GPE_ERR_INVALID and "GPE_POT_PRECOMPUTED" in str(ei.value)
        with pytest.raises(GPEError) as ei:                              # a sampler without terms on a precomputed config: the old message
            _bind_sampler(eng, "plain")
        assert ei.value.code == capi.GPE_ERR_INVALID and "a precomputed potential lives on fixed points" in str(ei.value)
        with pytest.raises(GPEError) as ei:                              # no terms, no array: the old message
            eng.bind_points(ctx["x"])
        assert ei.value.code == capi.GPE_ERR_INVALID and "d_V is NULL" in str(ei.value)
        with pytest.raises(GPEError) as ei:
            eng.bind_potential_terms([pot.lattice(1.0, (0.0, 0.0))])
        assert ei.value.code == capi.GPE_ERR_INVALID and "lattice" in str(ei.value) and eng.potential_terms() == []
        eng.bind_potential_terms(terms)
        with pytest.raises(GPEError) as ei:                              # d_V given with terms bound
            eng.bind_points(ctx["x"], V=np.zeros(ctx["N"], np.float32))
        assert ei.value.code == capi.GPE_ERR_INVALID and "terms are bound" in str(ei.value)
        _bind_sampler(eng, "plain")
        with pytest.raises(GPEError) as ei:                              # clearing under a sampler
            eng.clear_potential_terms()
        assert ei.value.code == capi.GPE_ERR_STATE and "sampler" in str(ei.value)
        eng.set_params(ctx["flat"])
        assert np.isfinite(eng.step()["loss"])
        eng.clear_sampler()
        _bind(eng, ctx)
        sc = eng.step()
        assert np.isfinite(sc["loss"])
        eng.clear_potential_terms()                                      # the bound set ran on the engine's V: it goes
        with pytest.raises(GPEError) as ei:
            eng.step()
        assert ei.value.code == capi.GPE_ERR_STATE
        _bind(eng, ctx, V=ctx["V"].astype(np.float32))                   # ... and the engine is what it was before the terms
        assert np.isfinite(eng.step()["loss"])
    finally:
        eng.close(); plain.close()
