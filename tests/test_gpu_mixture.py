"""Two-component mixture on the GPU (gpe_config.mixture: k_head_mix / k_seed_mix behind the n_out = 2 forward and reverse kernels)
against the fp64 reference tests/mixture_ref.py, which tests/test_mixture_reference_cpu.py holds to torch autograd.

Tolerances are those tests/test_gpu_parity.py applies to its complex-psi cases -- the same kernels with the same round-off: mu_a 2e-5,
loss / pde / bc 1e-4, norm 2e-4, gradient 5e-5 of max|g| and, per parameter block, helpers.BLOCK_TOL of the block's own maximum.  The
inputs (tests/mixture_cases.py) are such that a kernel without the cross term of the seeds would miss the gradient bound by a factor
of several hundred (asserted on the CPU)."""
import dataclasses
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import Engine, GPEConfig, GPEError, capi
from oracle import gpe_oracle as go
from tests import helpers as H
from tests import mixture_cases as mc
from tests import mixture_ref as mr

pytestmark = pytest.mark.gpu

PATHS = {"generic": gpe_pinn.PATH_GENERIC, "fused": gpe_pinn.PATH_FUSED, "auto": gpe_pinn.PATH_AUTO}
SCALAR_TOLS = (("mu1", 2e-5), ("mu2", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("bc", 1e-4), ("norm", 2e-4))
f64 = lambda a: None if a is None else np.asarray(a, np.float64)
dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def config(mp, path="auto", **kw):
    pb = mp.pb
    d = dict(layers=list(pb.layers), activation=pb.activation, kinetic_coeff=pb.kinetic_coeff, potential=pb.potential, pot_scale=pb.pot_scale,
             omega=tuple(pb.omega), perturb_scale=pb.perturb_scale, bc_nn_scale=pb.bc_nn_scale, w_pde=pb.w_pde, w_bc=pb.w_bc,
             w_norm=pb.w_norm, dx=pb.dx, n_global=pb.n_global, mixture=True, mix_g=tuple(mp.g), mix_norm=tuple(mp.n), path=PATHS[path])
    d.update(kw)
    return GPEConfig(**d)


def make_engine(mp, flat, x, x_bc=None, tgt=None, path="auto", q=None, total=None, **kw):
    eng = Engine(config(mp, path, **kw))
    try:
        eng.set_params(flat)
        eng.bind_points(dev(x))
        if x_bc is not None:
            eng.bind_boundary(dev(x_bc), None if tgt is None else dev(tgt))
        if q is not None:
            eng.bind_weights(dev(q), total)
    except Exception:
        eng.close()
        raise
    return eng


@contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def record(eng, sc):
    """the step's gpe_scalars record and gpe_mixture_scalars under the reference's names"""
    m = eng.mixture_scalars()
    assert sc["mu"] == m["mu1"] and sc["num"] == m["num1"] and sc["den"] == m["den1"] and sc["integral"] == m["integral1"]
    return dict(sc, **m)


def failures(got, grad, ref_sc, ref_grad, layers):
    bad = [f"{k} {got[k]:.9g} vs reference {ref_sc[k]:.9g}" for k, tol in SCALAR_TOLS
           if not abs(got[k] - ref_sc[k]) <= tol * max(abs(ref_sc[k]), 1e-6)]
    e = H.rel_err(grad, ref_grad)
    if not e < 5e-5:
        bad.append(f"gradient rel err {e:.3e}")
    return bad + H.block_failures(grad, ref_grad, layers)


_REF = {}


def reference(name):
    """the case's inputs and fp64 reference, computed once per module run and left unchanged"""
    if name not in _REF:
        mp, x, flat, x_bc, tgt, path = mc.case(name)
        sc, grad, fields = mr.loss_and_grad(mp, f64(flat), f64(x), f64(x_bc), f64(tgt))
        _REF[name] = dict(mp=mp, x=x, flat=flat, x_bc=x_bc, tgt=tgt, path=path, sc=sc, grad=grad, fields=fields)
    return _REF[name]


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_one_step_matches_the_reference(name):
    r = reference(name)
    mp = r["mp"]
    eng = make_engine(mp, r["flat"], r["x"], r["x_bc"], r["tgt"], r["path"])
    try:
        assert eng.active_path == PATHS[r["path"]]
        ak = eng.active_kernels
        assert ak["head"].startswith("k_head_mix<") and ak["seed"].startswith("k_seed_mix<") and "weighted" not in ak["head"], ak
        assert ",head>" not in ak["fwd"] and "seeds" not in ak["bwd"], ak
        rs, psi, res = eng.residual()
        assert np.abs(psi.cpu().numpy() - r["fields"]["psi"]).max() <= 5e-6 * np.abs(r["fields"]["psi"]).max() + 2e-6
        assert np.abs(res.cpu().numpy() - r["fields"]["residual"]).max() <= 2e-5 * np.abs(r["fields"]["residual"]).max() + 1e-5
        got = record(eng, eng.step())
        grad = eng.get_grad()
        print(name, {k: (got[k], r["sc"][k]) for k, _ in SCALAR_TOLS}, "gradient rel err", H.rel_err(grad, r["grad"]))
        bad = failures(got, grad, r["sc"], r["grad"], mp.pb.layers)
        assert not bad, bad
        assert abs(rs["loss"] - r["sc"]["loss"]) <= 1e-4 * abs(r["sc"]["loss"])
        new, _, _ = go.optimizer_step(go.OptState(lr0=1e-3), r["flat"], r["grad"], r["sc"]["loss"])
        d = np.abs(eng.get_params() - new)
        assert np.quantile(d, 0.99) < 2e-5 and d.max() < 2.1e-3
    finally:
        eng.close()


def _row_net(flat, layers, a):
    params = go.unflatten(np.asarray(flat, np.float64), layers)
    W, b = params[-1]
    return go.flatten(params[:-1] + [(W[a:a + 1], b[a:a + 1])]).astype(np.float32), list(layers[:-1]) + [1]


@pytest.mark.parametrize("name", ["fused_2d_64x3_N1025", "generic_1d_48x2_N37"])
def test_decoupled_components_equal_scalar_engines(name):
    """g12 = 0: component a's u, H u - mu u and mu_a are those of a scalar engine on the network cut to output row a"""
    layers, N, path, act = mc.CASES[name]
    x, flat, _, _ = mc.inputs(layers, N)
    g = (mc.G[0], mc.G[1], 0.0)
    mp = mc.problem(layers, N, act, g=g, norms=(1.0, 1.0), w_bc=0.0)
    eng = make_engine(mp, flat, x, path=path)
    try:
        _, psi, res = eng.residual()
        m = eng.mixture_scalars()
        psi, res = psi.cpu().numpy(), res.cpu().numpy()
    finally:
        eng.close()
    for a in range(2):
        fa, la = _row_net(flat, layers, a)
        pb = mp.pb
        sca = Engine(GPEConfig(layers=la, activation=act, kinetic_coeff=pb.kinetic_coeff, pot_scale=pb.pot_scale, gamma=g[a], p=3, w_bc=0.0,
                               w_norm=pb.w_norm, dx=pb.dx, path=PATHS[path]))
        try:
            sca.set_params(fa)
            sca.bind_points(dev(x))
            ss, spsi, sres = sca.residual()
        finally:
            sca.close()
        spsi, sres = spsi.cpu().numpy()[:, 0], sres.cpu().numpy()[:, 0]
        assert np.abs(psi[:, a] - spsi).max() <= 5e-6 * np.abs(spsi).max() + 2e-6
        assert np.abs(res[:, a] - sres).max() <= 2e-5 * np.abs(sres).max() + 1e-5
        assert abs(m[f"mu{a + 1}"] - ss["mu"]) <= 2e-5 * abs(ss["mu"])
        assert abs(m[f"integral{a + 1}"] - ss["integral"]) <= 2e-5 * abs(ss["integral"])


@pytest.mark.parametrize("name", ["fused_2d_64x3_N49", "generic_3d_40_N37"])
def test_integer_weights_equal_the_duplicated_batch(name):
    """Integer weights (zeros among them): the weighted instances against the reference with weights, and the weighted step against the
    unweighted step on the batch with row i repeated q_i times"""
    r = reference(name)
    mp, x = r["mp"], r["x"]
    N = x.shape[0]
    q = np.random.default_rng(3).integers(0, 4, N).astype(np.float32)
    W = float(q.sum())
    sc, grad, _ = mr.loss_and_grad(mp, f64(r["flat"]), f64(x), f64(r["x_bc"]), f64(r["tgt"]), q=f64(q))
    eng = make_engine(mp, r["flat"], x, r["x_bc"], r["tgt"], r["path"], q=q)
    try:
        ak = eng.active_kernels
        assert "k_head_mix" in ak["head"] and "weighted" in ak["head"] and "weighted" in ak["seed"], ak
        got = record(eng, eng.step())
        g1 = eng.get_grad()
    finally:
        eng.close()
    bad = failures(got, g1, sc, grad, mp.pb.layers)
    assert not bad, bad
    idx = np.repeat(np.arange(N), q.astype(np.int64))
    mpd = dataclasses.replace(mp, pb=dataclasses.replace(mp.pb, n_global=int(W)))
    dup = make_engine(mpd, r["flat"], x[idx], r["x_bc"], r["tgt"], r["path"])
    try:
        gd = record(dup, dup.step())
        g2 = dup.get_grad()
    finally:
        dup.close()
    for k in ("num1", "den1", "num2", "den2"):                 # fp64 sums of the same fp32 terms, in another order
        assert abs(got[k] - gd[k]) <= 1e-12 * abs(gd[k]), k
    for k, tol in SCALAR_TOLS:
        assert abs(got[k] - gd[k]) <= tol * max(abs(gd[k]), 1e-6), k
    assert H.rel_err(g1, g2) < 5e-5


def dp_step(engs):
    """the three phases on every rank with both exchanges summed by hand, in float64, in rank order (tests/test_gpu_dp_matrix.py)"""
    for e in engs:
        e.step_begin()
    tot = torch.zeros_like(engs[0].exchange_sums, dtype=torch.float64)
    for e in engs:
        tot += e.exchange_sums
    for e in engs:
        e.exchange_sums.copy_(tot)
        e.step_backward()
    gt = torch.zeros_like(engs[0].exchange_grad, dtype=torch.float64)
    for e in engs:
        gt += e.exchange_grad.to(torch.float64)
    g32 = gt.to(torch.float32)
    for e in engs:
        e.exchange_grad.copy_(g32)
        e.step_update()


@pytest.mark.parametrize("name", ["fused_2d_64x3_N1025", "generic_2d_64x2_N1025", "wide_3d_256x2_N300"])
def test_three_ranks_by_hand_match_the_reference_on_all_points(name):
    r = reference(name)
    mp, x = r["mp"], r["x"]
    N = x.shape[0]
    mpn = dataclasses.replace(mp, pb=dataclasses.replace(mp.pb, n_global=N))
    engs = []
    try:
        for lo, hi in H.dp_cuts(3, N):
            engs.append(make_engine(mpn, r["flat"], x[lo:hi], r["x_bc"], r["tgt"], r["path"], world_size=3))
        assert engs[0].exchange_sums.numel() == 12                    # (num_2, den_2) ride in the first message as it was
        dp_step(engs)
        for e in engs:
            e.synchronize()
        recs = [record(e, e.read_scalars()) for e in engs]
        grads = [e.get_grad() for e in engs]
        params = [e.get_params() for e in engs]
    finally:
        for e in engs:
            e.close()
    bad = failures(recs[0], grads[0], r["sc"], r["grad"], mp.pb.layers)
    assert not bad, bad
    for k in range(1, 3):                                             # every rank applied the same update to the same record
        np.testing.assert_array_equal(params[k], params[0])
        assert recs[k]["mu2"] == recs[0]["mu2"] and recs[k]["loss"] == recs[0]["loss"]


RUN_CASE = ([2, 64, 64, 64, 2], 777)


def _run_engine(env=None, clip_norm=1.0):
    layers, N = RUN_CASE
    x, flat, x_bc, tgt = mc.inputs(layers, N, seed=4)
    with environment(env or {}):
        return make_engine(mc.problem(layers, N), flat, x, x_bc, tgt, "auto", clip_norm=clip_norm), (layers, N, x, flat, x_bc, tgt)


def test_run_with_graph_replay_equals_repeated_steps_bit_for_bit():
    """20 steps: gpe_run (777 points: captured graphs of 8 steps, the remainder by plain launches) against 20 calls of gpe_step.  One
    workgroup of k_head_mix / k_seed_mix at this size: one atomic per sum, so the step repeats bit for bit."""
    a, _ = _run_engine()
    b, _ = _run_engine()
    try:
        a.run(20)
        a.synchronize()
        for _ in range(20):
            last = b.step()
        np.testing.assert_array_equal(a.get_params(), b.get_params())
        ra = a.read_scalars()
        assert ra["step"] == 20 and ra["loss"] == last["loss"] and a.mixture_scalars() == b.mixture_scalars()
    finally:
        a.close(); b.close()


# the forms of the update kernel the switch table lists (tests/switch_table.py, "update kernel forms"); the default is the register-cached one
UPDATE_FORMS = {"two_pass": {"GPE_UPDATE_CACHE": "0"}, "fused_into_reduction": {"GPE_FUSE_UPDATE": "1"}, "split": {"GPE_SPLIT_UPDATE": "1"},
                "multi": {"GPE_UPDATE_MULTI_MIN": "1"}}


@pytest.mark.parametrize("form", sorted(UPDATE_FORMS))
def test_update_kernel_forms_agree_bit_for_bit_on_a_mixture_step(form):
    """Without clipping (the forms that add |g|^2 in another order then scale by the same coef = 1): parameters, Adam moments, the record
    and gpe_mixture_scalars of two steps are bit-identical to the default form's."""
    out = []
    for env in ({}, UPDATE_FORMS[form]):
        eng, _ = _run_engine(env, clip_norm=0.0)
        try:
            eng.step()
            sc = eng.step()
            out.append((eng.get_params(), eng.get_adam_state(), {k: sc[k] for k in ("loss", "pde", "bc", "norm", "mu", "integral", "step")},
                        eng.mixture_scalars()))
        finally:
            eng.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1][0], out[1][1][0])
    np.testing.assert_array_equal(out[0][1][1], out[1][1][1])
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3]


def test_six_optimiser_steps_follow_the_reference():
    """loss of step k within 1e-3 (1 + k) of the reference stepped with oracle.optimizer_step (the bound of tools/fuzz_parity.py)"""
    eng, (layers, N, x, flat, x_bc, tgt) = _run_engine()
    mp = mc.problem(layers, N)
    st, th = go.OptState(lr0=1e-3), flat.copy()
    try:
        for k in range(6):
            sc, grad, _ = mr.loss_and_grad(mp, f64(th), f64(x), f64(x_bc), f64(tgt))
            got = eng.step()
            print("step", k, got["loss"], sc["loss"])
            assert abs(got["loss"] - sc["loss"]) <= 1e-3 * (1 + k) * abs(sc["loss"]), (k, got["loss"], sc["loss"])
            th, _, _ = go.optimizer_step(st, th, grad, sc["loss"])
    finally:
        eng.close()


def test_set_mixture_takes_effect_at_the_next_step():
    eng, (layers, N, x, flat, x_bc, tgt) = _run_engine()
    g2 = (2.0, 5.0, -1.5)
    try:
        eng.run(8)                                                     # (a captured graph exists when the couplings change)
        eng.synchronize()
        th = eng.get_params()
        eng.set_mixture(*g2)
        assert eng.cfg.mix_g == g2
        eng.run(8)
        eng.synchronize()
        first = eng.read_history(9, 1)[0]
        sc, _, _ = mr.loss_and_grad(mc.problem(layers, N, g=g2), f64(th), f64(x), f64(x_bc), f64(tgt))
        old, _, _ = mr.loss_and_grad(mc.problem(layers, N), f64(th), f64(x), f64(x_bc), f64(tgt))
        assert abs(first["loss"] - sc["loss"]) <= 1e-4 * abs(sc["loss"]) and abs(first["mu"] - sc["mu1"]) <= 2e-5 * abs(sc["mu1"])
        assert abs(old["loss"] - sc["loss"]) > 1e-2 * abs(sc["loss"])           # (the two couplings are told apart by far more than the bound)
        with pytest.raises(GPEError):
            eng.set_mixture(1.0, float("nan"), 0.0)
    finally:
        eng.close()


def test_mixture_scalars_equal_the_host_side_sums_of_the_residual_fields():
    r = reference("fused_2d_64x3_N1025")
    mp = r["mp"]
    eng = make_engine(mp, r["flat"], r["x"], r["x_bc"], r["tgt"], r["path"])
    try:
        sc, psi, res = eng.residual()
        m = eng.mixture_scalars()
    finally:
        eng.close()
    u32, r32 = psi.cpu().numpy(), res.cpu().numpy()
    u, rr = u32.astype(np.float64), r32.astype(np.float64)
    for a in (0, 1):
        den = float((u32[:, a] * u32[:, a]).astype(np.float64).sum())  # the kernel's terms: fp32 products, widened, added in fp64
        assert abs(m[f"den{a + 1}"] - den) <= 1e-9 * den
        assert m[f"integral{a + 1}"] == float(np.float32(m[f"den{a + 1}"]) * np.float32(mp.pb.dx))
        assert m[f"mu{a + 1}"] == float(np.float32(m[f"num{a + 1}"] / m[f"den{a + 1}"]))
        # H u is not among the fields: rebuilt from r_a = H_a u_a - mu_a u_a it carries the two fp32 roundings of that line
        Hu = rr[:, a] + m[f"mu{a + 1}"] * u[:, a]
        num = float((u[:, a] * Hu).sum())
        bound = 4 * 2.0 ** -24 * float((np.abs(u[:, a]) * (np.abs(rr[:, a]) + abs(m[f"mu{a + 1}"]) * np.abs(u[:, a]))).sum())
        assert abs(m[f"num{a + 1}"] - num) <= bound + 1e-9 * abs(num)
    nrm = sum((m[f"integral{a + 1}"] - float(np.float32(mp.n[a]))) ** 2 for a in (0, 1))
    assert abs(sc["norm"] - nrm) <= 1e-9 * nrm
    sr2 = float((r32 * r32).astype(np.float64).sum())
    assert abs(sc["sum_r2"] - sr2) <= 1e-6 * sr2                      # (the record keeps sum r^2 as the fp32 tail of the gradient message)


def test_state_refusals_of_a_mixture_engine():
    r = reference("fused_2d_64x3_N37")
    eng = make_engine(r["mp"], r["flat"], r["x"], r["x_bc"], r["tgt"], r["path"])
    xs = dev(r["x"])
    try:
        for what, call in (("observables", lambda: eng.observables()), ("observables on points", lambda: eng.observables(xs)),
                           ("monitor", lambda: eng.bind_monitor(xs, 2)), ("keeper", lambda: eng.bind_keeper("res_rms")),
                           ("orth", lambda: eng.bind_orth(0, torch.zeros(37, device="cuda"))),
                           ("orth_state", lambda: eng.bind_orth_state(0, r["flat"])),
                           ("eval_density", lambda: eng.eval_density(xs, 0.1))):
            with pytest.raises(GPEError) as ex:
                call()
            assert ex.value.code == capi.GPE_ERR_STATE, (what, str(ex.value))
        sc = eng.step()                                                # ... and the engine steps on
        assert sc["step"] == 1.0 and np.isfinite(sc["loss"])
    finally:
        eng.close()
    scalar = Engine(GPEConfig(layers=[2, 64, 64, 1]))
    try:
        for call in (lambda: scalar.set_mixture(1.0, 1.0, 0.5), lambda: scalar.mixture_scalars()):
            with pytest.raises(GPEError) as ex:
                call()
            assert ex.value.code == capi.GPE_ERR_STATE
    finally:
        scalar.close()
