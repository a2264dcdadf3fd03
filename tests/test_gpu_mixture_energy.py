"""The mixture energy term on the GPU (gpe_mixture_energy_weight / gpe_mixture_energy: k_head_mix<.., energy> / k_seed_mix<.., energy>
behind the n_out = 2 forward and reverse kernels) against the fp64 reference tests/mixture_energy_ref.py, which
tests/test_mixture_energy_reference_cpu.py holds to torch autograd.

Scalar tolerances are those of tests/test_gpu_mixture.py (mu_a 2e-5; loss, pde, bc 1e-4; norm 2e-4; gradient 5e-5 of max|g| plus
helpers.BLOCK_TOL per parameter block); E is held to 1e-4 relative, the bound tests/test_gpu_parity.py applies to `riesz`, and so are the
sums E is formed from.  Inputs are the cases of tests/mixture_cases.py, the weights mixture_energy_ref.W_E: on them a kernel without the
delta_a term or without the first-derivative seeds misses the gradient bound by a factor of several hundred (asserted on the CPU)."""
import dataclasses

import numpy as np
import pytest
import torch

from gpe_pinn import Engine, GPEConfig, GPEError, capi
from oracle import gpe_oracle as go
from tests import helpers as H
from tests import mixture_cases as mc
from tests import mixture_energy_ref as me
from tests import mixture_flow_1d as mf
from tests import test_gpu_mixture as tm

pytestmark = pytest.mark.gpu

f64, dev = tm.f64, tm.dev
E_TOL = 1e-4
CASES = sorted(me.W_E)
STEP_CASES = [n for n in CASES if n != "fused_2d_64x3_N49"]         # the nine cases of the one-step test (N49 carries the weighted / live tests)


# g_bwd_weight_mfma (64-wide layers of the generic set, more than one chunk of points) adds its split-K partial weight gradients with
# fp32 atomics: the order varies from launch to launch, so not even two untouched engines repeat each other's step bit for bit there
FLOAT_ATOMIC_GRADIENT = {"generic_2d_64x2_N1025"}

_REF = {}


def reference(name):
    """the case's inputs and fp64 reference at its weight, computed once per module run and left unchanged"""
    if name not in _REF:
        mp, x, flat, x_bc, tgt, path = mc.case(name)
        sc, grad, _ = me.loss_and_grad(mp, me.W_E[name], f64(flat), f64(x), f64(x_bc), f64(tgt))
        _REF[name] = dict(mp=mp, x=x, flat=flat, x_bc=x_bc, tgt=tgt, path=path, sc=sc, grad=grad, w=me.W_E[name])
    return _REF[name]


def engine(r, w=None, **kw):
    eng = tm.make_engine(r["mp"], r["flat"], r["x"], r["x_bc"], r["tgt"], r["path"], **kw)
    if w is not None:
        eng.set_mixture_energy(w)
    return eng


def failures(got, grad, ref_sc, ref_grad, layers):
    bad = tm.failures(got, grad, ref_sc, ref_grad, layers)
    if not abs(got["riesz"] - ref_sc["E"]) <= E_TOL * abs(ref_sc["E"]):
        bad.append(f"E {got['riesz']:.9g} vs reference {ref_sc['E']:.9g}")
    return bad


def energy_failures(got, ref_sc):
    return [f"{k} {got[k]:.9g} vs reference {ref_sc[k]:.9g}" for k in me.ENERGY_FIELDS if not abs(got[k] - ref_sc[k]) <= E_TOL * abs(ref_sc[k])]


@pytest.mark.parametrize("name", STEP_CASES)
def test_one_step_with_the_term_on_matches_the_reference(name):
    r = reference(name)
    eng = engine(r, r["w"])
    try:
        ak = eng.active_kernels
        assert ak["head"].startswith("k_head_mix<") and ak["head"].endswith(",energy>") and ak["seed"].startswith("k_seed_mix<") \
            and ak["seed"].endswith(",energy>") and "weighted" not in ak["head"], ak
        got = tm.record(eng, eng.step())
        grad = eng.get_grad()
        print(name, {k: (got[k], r["sc"][k]) for k, _ in tm.SCALAR_TOLS}, "E", (got["riesz"], r["sc"]["E"]), "gradient rel err", H.rel_err(grad, r["grad"]))
        bad = failures(got, grad, r["sc"], r["grad"], r["mp"].pb.layers)
        assert not bad, bad
    finally:
        eng.close()


@pytest.mark.parametrize("name", STEP_CASES)
def test_mixture_energy_reads_the_reference_and_leaves_the_engine_alone(name):
    r = reference(name)
    a, b = engine(r), engine(r, r["w"])
    try:
        e0 = a.mixture_energy()                                        # at w_E = 0 ...
        a.set_mixture_energy(r["w"])
        e1 = a.mixture_energy()                                        # ... and with the term on
        print(name, e0, e1)
        assert not energy_failures(e0, r["sc"]) and not energy_failures(e1, r["sc"]), (energy_failures(e0, r["sc"]), energy_failures(e1, r["sc"]))
        np.testing.assert_array_equal(a.get_params(), r["flat"])
        a.step(); b.step()
        th, adam = a.get_params(), a.get_adam_state()
        a.mixture_energy()                                             # (a second detour, between two steps)
        np.testing.assert_array_equal(a.get_params(), th)
        for m0, m1 in zip(adam[:2], a.get_adam_state()[:2]):
            np.testing.assert_array_equal(m0, m1)
        ra, rb = a.step(), b.step()
        if name in FLOAT_ATOMIC_GRADIENT:          # two untouched engines differ in the last bit here: held to a few ulp instead
            np.testing.assert_allclose(a.get_params(), b.get_params(), rtol=2e-6, atol=1e-7)
            for k in ("loss", "pde", "bc", "norm", "mu", "riesz", "grad_norm"):
                assert abs(ra[k] - rb[k]) <= 1e-6 * abs(rb[k]), k
            return
        np.testing.assert_array_equal(a.get_params(), b.get_params())
        for ma, mb in zip(a.get_adam_state()[:2], b.get_adam_state()[:2]):
            np.testing.assert_array_equal(ma, mb)
        assert ra == rb and a.mixture_scalars() == b.mixture_scalars(), (ra, rb)
    finally:
        a.close(); b.close()


def test_off_means_off():
    """An engine that set w_E and set it back repeats the untouched engine's next three steps bit for bit, through the parent's kernels"""
    r = reference("fused_2d_64x3_N1025")
    a, b = engine(r), engine(r)
    try:
        plain = b.active_kernels
        assert plain["head"] == "k_head_mix<4,1>" and plain["seed"] == "k_seed_mix<4,1>", plain
        a.set_mixture_energy(r["w"])
        assert a.active_kernels["head"] == "k_head_mix<4,1,energy>" and a.active_kernels["seed"] == "k_seed_mix<4,1,energy>"
        a.set_mixture_energy(0.0)
        assert a.active_kernels == plain
        for k in range(3):
            ra, rb = a.step(), b.step()
            assert ra == rb and ra["riesz"] == 0.0, (k, ra, rb)
            np.testing.assert_array_equal(a.get_grad(), b.get_grad())
            np.testing.assert_array_equal(a.get_params(), b.get_params())
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("name", ["fused_2d_64x3_N49", "generic_3d_40_N37"])
def test_integer_weights_equal_the_duplicated_batch(name):
    r = reference(name)
    mp, x, w = r["mp"], r["x"], r["w"]
    N = x.shape[0]
    q = np.random.default_rng(3).integers(1, 4, N).astype(np.float32)
    W = float(q.sum())
    sc, grad, _ = me.loss_and_grad(mp, w, f64(r["flat"]), f64(x), f64(r["x_bc"]), f64(r["tgt"]), q=f64(q))
    eng = engine(r, w, q=q)
    try:
        ak = eng.active_kernels
        assert ak["head"].endswith(",weighted,energy>") and ak["seed"].endswith(",weighted,energy>"), ak
        en = eng.mixture_energy()
        got = tm.record(eng, eng.step())
        g1 = eng.get_grad()
    finally:
        eng.close()
    bad = failures(got, g1, sc, grad, mp.pb.layers) + energy_failures(en, sc)
    assert not bad, bad
    idx = np.repeat(np.arange(N), q.astype(np.int64))
    mpd = dataclasses.replace(mp, pb=dataclasses.replace(mp.pb, n_global=int(W)))
    dup = tm.make_engine(mpd, r["flat"], x[idx], r["x_bc"], r["tgt"], r["path"])
    try:
        dup.set_mixture_energy(w)
        end = dup.mixture_energy()
        gd = tm.record(dup, dup.step())
        g2 = dup.get_grad()
    finally:
        dup.close()
    for k in me.ENERGY_FIELDS[1:]:                                    # fp64 sums of the same fp32 terms, in another order
        assert abs(en[k] - end[k]) <= 1e-12 * abs(end[k]), k
    for k, tol in tm.SCALAR_TOLS + (("riesz", E_TOL),):
        assert abs(got[k] - gd[k]) <= tol * max(abs(gd[k]), 1e-6), k
    assert H.rel_err(g1, g2) < 5e-5


@pytest.mark.parametrize("name", ["fused_2d_64x3_N1025", "generic_2d_64x2_N1025", "wide_3d_256x2_N300"])
def test_three_ranks_by_hand_match_the_reference_on_all_points(name):
    r = reference(name)
    mp, x = r["mp"], r["x"]
    N = x.shape[0]
    mpn = dataclasses.replace(mp, pb=dataclasses.replace(mp.pb, n_global=N))
    engs = []
    try:
        for lo, hi in H.dp_cuts(3, N):
            engs.append(tm.make_engine(mpn, r["flat"], x[lo:hi], r["x_bc"], r["tgt"], r["path"], world_size=3))
            engs[-1].set_mixture_energy(r["w"])
        assert engs[0].exchange_sums.numel() == 12                    # the five energy sums ride in the first message as it was
        tm.dp_step(engs)
        for e in engs:
            e.synchronize()
        recs = [tm.record(e, e.read_scalars()) for e in engs]
        grads = [e.get_grad() for e in engs]
        params = [e.get_params() for e in engs]
    finally:
        for e in engs:
            e.close()
    bad = failures(recs[0], grads[0], r["sc"], r["grad"], mp.pb.layers)
    assert not bad, bad
    for k in range(1, 3):                                             # every rank applied the same update to the same record
        np.testing.assert_array_equal(params[k], params[0])
        assert recs[k]["riesz"] == recs[0]["riesz"] and recs[k]["loss"] == recs[0]["loss"]


# ---- live engine -------------------------------------------------------------------------------------------------------------------------
LIVE = "fused_2d_64x3_N49"


def test_run_with_graph_replay_equals_repeated_steps_across_a_weight_change():
    """8 steps plain, the weight set, 17 steps with the term (gpe_run: two replays of the rebuilt 8-step graph and one plain launch), the
    weight cleared, 8 more -- against the same sequence by gpe_step; and the step behind each change is the changed problem's"""
    r = reference(LIVE)
    mp, w = r["mp"], r["w"]
    a, b = engine(r), engine(r)
    try:
        a.run(8); a.synchronize()
        th = a.get_params()
        a.set_mixture_energy(w)
        a.run(17); a.synchronize()
        th2 = a.get_params()
        a.set_mixture_energy(0.0)
        a.run(8); a.synchronize()
        for n, wk in ((8, w), (17, 0.0), (8, None)):
            for _ in range(n):
                last = b.step()
            if wk is not None:
                b.set_mixture_energy(wk)
        np.testing.assert_array_equal(a.get_params(), b.get_params())
        ra = a.read_scalars()
        assert ra == last and ra["step"] == 33.0
        first = a.read_history(9, 1)[0]
        sc, _, _ = me.loss_and_grad(mp, w, f64(th), f64(r["x"]), f64(r["x_bc"]), f64(r["tgt"]))
        assert abs(first["loss"] - sc["loss"]) <= 1e-4 * abs(sc["loss"]) and abs(first["riesz"] - sc["E"]) <= E_TOL * abs(sc["E"])
        assert abs(w * sc["E"]) > 1e-2 * abs(sc["loss"])               # (the term is told from its absence by far more than the bound)
        back = a.read_history(26, 1)[0]
        sc0, _, _ = me.loss_and_grad(mp, 0.0, f64(th2), f64(r["x"]), f64(r["x_bc"]), f64(r["tgt"]))
        assert abs(back["loss"] - sc0["loss"]) <= 1e-4 * abs(sc0["loss"]) and back["riesz"] == 0.0
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("form", sorted(tm.UPDATE_FORMS))
def test_update_kernel_forms_agree_bit_for_bit_with_the_term_on(form):
    r = reference(LIVE)
    out = []
    for env in ({}, tm.UPDATE_FORMS[form]):
        with tm.environment(env):
            eng = engine(r, r["w"], clip_norm=0.0)
        try:
            eng.step()
            sc = eng.step()
            assert sc["riesz"] != 0.0 and sc["step"] == 2.0
            out.append((eng.get_params(), eng.get_adam_state(), {k: sc[k] for k in ("loss", "pde", "bc", "norm", "mu", "integral", "riesz", "step")},
                        eng.mixture_scalars()))
        finally:
            eng.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1][0], out[1][1][0])
    np.testing.assert_array_equal(out[0][1][1], out[1][1][1])
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3]


def test_refusals():
    r = reference("fused_2d_64x3_N37")
    eng = engine(r)
    try:
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(GPEError) as ex:
                eng.set_mixture_energy(bad)
            assert ex.value.code == capi.GPE_ERR_INVALID
        with pytest.raises(GPEError) as ex:                              # the scalar Riesz weight stays refused
            eng.set_loss_weights(1.0, 10.0, 20.0, w_riesz=1.0)
        assert ex.value.code == capi.GPE_ERR_INVALID
        assert eng.active_kernels["head"] == "k_head_mix<4,1>"          # ... and a refused weight changed nothing
    finally:
        eng.close()
    scalar = Engine(GPEConfig(layers=[2, 64, 64, 1]))
    try:
        for call in (lambda: scalar.set_mixture_energy(1.0), lambda: scalar.mixture_energy()):
            with pytest.raises(GPEError) as ex:
                call()
            assert ex.value.code == capi.GPE_ERR_STATE
    finally:
        scalar.close()


W_E_RUN = 512.0


def test_six_optimiser_steps_with_the_term_on_follow_the_reference():
    """loss of step k within 1e-3 (1 + k) of the reference stepped with oracle.optimizer_step (tests/test_gpu_mixture.py's bound)"""
    eng, (layers, N, x, flat, x_bc, tgt) = tm._run_engine()
    mp = mc.problem(layers, N)
    st, th = go.OptState(lr0=1e-3), flat.copy()
    try:
        eng.set_mixture_energy(W_E_RUN)
        for k in range(6):
            sc, grad, _ = me.loss_and_grad(mp, W_E_RUN, f64(th), f64(x), f64(x_bc), f64(tgt))
            got = eng.step()
            print("step", k, got["loss"], sc["loss"], got["riesz"], sc["E"])
            assert abs(got["loss"] - sc["loss"]) <= 1e-3 * (1 + k) * abs(sc["loss"]), (k, got["loss"], sc["loss"])
            assert W_E_RUN * sc["E"] > 0.05 * sc["loss"]                # (the term carries a visible share of the loss that is followed)
            th, _, _ = go.optimizer_step(st, th, grad, sc["loss"])
    finally:
        eng.close()


# ---- demixing: the DESIGN run ------------------------------------------------------------------------------------------------------------
DEMIX = dict(layers=[1, 64, 64, 64, 2], points=1024, half=8.0, g=10.0, g12=14.0, pretrain=1000, steps=8000, lr=1e-3, w_E=1.0)


def _demix_run(w_E):
    """1D, components pre-trained on Gaussians +-0.5 apart, then `steps` steps at the full couplings -> E of the state reached"""
    from bench import reference_init
    d = DEMIX
    N, L = d["points"], d["half"]
    x = np.linspace(-L, L, N).reshape(-1, 1)
    eng = Engine(GPEConfig(layers=d["layers"], kinetic_coeff=0.5, pot_scale=0.5, dx=2 * L / (N - 1), w_pde=1.0, w_bc=10.0, w_norm=20.0, lr=d["lr"],
                           clip_norm=1.0, mixture=True, mix_g=(0.0, 0.0, 0.0), mix_norm=(0.5, 0.5), n_global=N))
    try:
        eng.set_params(reference_init(d["layers"], seed=1))
        eng.bind_points(dev(x))
        eng.bind_boundary(dev(np.array([[-L], [L]])))
        tgt = np.stack([np.sqrt(0.5) * np.pi ** -0.25 * np.exp(-0.5 * (x[:, 0] + s) ** 2) for s in (0.5, -0.5)], axis=1)
        eng.bind_target(dev(tgt))
        for _ in range(d["pretrain"]):
            eng.mse_step()
        eng.reset_optimizer(d["lr"])
        eng.set_mixture(d["g"], d["g"], d["g12"])
        eng.set_mixture_energy(w_E)
        eng.run(d["steps"])
        eng.synchronize()
        return eng.mixture_energy()["E"], eng.read_scalars()
    finally:
        eng.close()


def test_training_with_the_energy_term_demixes_and_without_it_does_not():
    """g = 10, g12 = 14, n = 1/2 each: the separated ground state lies at E_sep, the symmetric (unstable) stationary state at E_sym
    (tests/mixture_flow_1d.py).  Trained with the energy term the state ends below their midpoint; the same run on the residual loss
    alone ends above it -- the behaviour DESIGN section 4 recorded.  Measured on the MI355X: E = 2.1454 with w_E = 1, 2.1802 without,
    midpoint 2.1565 (E_sym 2.17303, E_sep 2.13988)."""
    E_sym, E_sep = mf.sym_and_sep(DEMIX["g"], DEMIX["g12"])
    mid = 0.5 * (E_sym + E_sep)
    E_on, sc_on = _demix_run(DEMIX["w_E"])
    E_off, sc_off = _demix_run(0.0)
    print("E_sym", E_sym, "E_sep", E_sep, "midpoint", mid, "E with the term", E_on, "loss", sc_on["loss"], "E without", E_off, "loss", sc_off["loss"])
    assert E_sep < E_sym
    assert E_on < mid, (E_on, mid)
    assert E_off > mid, (E_off, mid)
