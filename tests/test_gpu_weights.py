"""Per-point quadrature weights (gpe_bind_weights) and the graded stratified sampler (gpe_bind_sampler_graded) on the GPU.

The reference of every weighted step is tests/weighted_ref.py: the fp64 oracle's own two-phase protocol with one point per shard, which
tests/test_weights_cpu.py ties to the oracle on the duplicated batch.  Tolerances of a step are those of test_step_matches_oracle
(mu 2e-5, loss terms 1e-4, norm 2e-4, gradient 5e-5 of max|g|)."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from gpe_pinn import Engine, GPEError, capi
from gpe_pinn import sampler as S
from oracle import gpe_oracle as go
from tests import helpers as H
from tests.test_gpu_dp_matrix import dp_step
from tests.test_gpu_orth_states import _frozen, _oracle_psi
from tests.test_gpu_parity import PATHS, cfg_from_problem, close, make_engine
from tests.weighted_ref import duplicated, weighted_loss_and_grad

pytestmark = pytest.mark.gpu

SCALAR_TOLS = (("mu", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("bc", 1e-4), ("norm", 2e-4), ("orth", 1e-4), ("riesz", 1e-4), ("reg", 1e-4),
               ("den", 2e-4), ("integral", 2e-4), ("sum_r2", 1e-4))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ---- 1. one step against the weighted reference ---------------------------------------------------------------------------------------
# (Problem kwargs, weight scale of the parameters, kernel sets).  dx: about 1 / (mean q * N) times the box, so that the norm integral is O(1)
FLAVOURS = {
    "2d_plain": (dict(layers=[2, 64, 64, 64, 1], gamma=50.0), 0.3, ("generic", "fused")),
    "1d_base_merged_bc": (dict(layers=[1, 32, 32, 1], gamma=2.0, base_mode=1), 0.3, ("generic", "fused")),
    "2d_riesz_variational": (dict(layers=[2, 64, 64, 64, 1], gamma=100.0, w_riesz=2.0, riesz_kind=go.RIESZ_VARIATIONAL), 0.3, ("generic", "fused")),
    "2d_energy_lambda_regs": (dict(layers=[2, 64, 64, 64, 1], gamma=100.0, kinetic_coeff=1.0, pot_scale=1.0, w_norm=0.0,
                                   lambda_kind=go.LAMBDA_ENERGY, w_reg_f=1.0, w_reg_lam=1.0), 0.3, ("generic", "fused")),
    "2d_orth": (dict(layers=[2, 64, 64, 64, 1], gamma=50.0, w_orth=3.0), 0.3, ("generic", "fused")),
    "2d_complex_rot_128": (dict(layers=[2, 128, 128, 2], complex_psi=True, gamma=30.0, omega_rot=0.8), 0.15, ("generic", "fused")),
    "3d_128x3": (dict(layers=[3, 128, 128, 128, 1], gamma=100.0, omega=(1.0, 1.4, 2.0)), 0.15, ("generic", "fused")),
}
SIZES = (37, 1025)          # less than one wave; two head workgroups, the second holding one point
_REF = {}


def weights_of(N, seed=3):
    """random fp32 in [0.25, 4), every seventh entry 0 (rows 3, 10, ...: a one-point shard of row 0 keeps a weight)"""
    q = np.random.default_rng(seed).uniform(0.25, 4.0, N).astype(np.float32)
    q[q >= 4.0] = 3.5
    q[3::7] = 0.0
    return q


def case(name, N):
    """inputs and fp64 reference of one (flavour, N), built once per module run and left unchanged"""
    if (name, N) in _REF:
        return _REF[name, N]
    kw, scale, _ = FLAVOURS[name]
    d = kw["layers"][0]
    rng = np.random.default_rng(17)
    x = (np.linspace(-6, 6, N).reshape(-1, 1) if d == 1 else rng.uniform(-3, 3, (N, d))).astype(np.float32)
    flat = (rng.normal(0, 1, go.param_count(kw["layers"])) * scale).astype(np.float32)
    x_bc = np.array([[-6.0], [6.0]], np.float32) if name == "1d_base_merged_bc" else None
    orth = (np.exp(-0.5 * (x.astype(np.float64) ** 2).sum(1)) * x[:, 0])[None, :].astype(np.float32) if name == "2d_orth" else None
    q = weights_of(N)
    dx = 1.0 if name == "2d_energy_lambda_regs" else float(np.float32((12.0 if d == 1 else 6.0 ** d) / q.sum(dtype=np.float64)))
    pb = go.Problem(**kw, dx=dx) if x_bc is not None else go.Problem(**kw, dx=dx, w_bc=0.0)
    o64 = None if orth is None else orth.astype(np.float64)
    ref = weighted_loss_and_grad(pb, flat, x, q, None if x_bc is None else x_bc.astype(np.float64), orth=o64)
    _REF[name, N] = dict(pb=pb, x=x, flat=flat, x_bc=x_bc, orth=orth, q=q, ref=ref)
    return _REF[name, N]


def weighted_engine(c, path="fused", **kw):
    eng = make_engine(c["pb"], c["flat"], c["x"], c["x_bc"], path=PATHS[path], **kw)
    if c["orth"] is not None:
        eng.bind_orth(0, dev(c["orth"][0]))
    return eng


def check_scalars(sc, osc, keys=SCALAR_TOLS):
    for k, tol in keys:
        if k in osc:
            assert abs(sc[k] - osc[k]) <= tol * max(abs(osc[k]), 1e-6), (k, sc[k], osc[k])


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name,path", [(n, p) for n, (_, _, paths) in FLAVOURS.items() for p in paths])
def test_weighted_step_matches_the_weighted_reference(name, path, N):
    c = case(name, N)
    osc, ograd, fields = c["ref"]
    eng = weighted_engine(c, path)
    assert eng.active_path == PATHS[path]
    eng.bind_weights(dev(c["q"]))
    assert "weighted" in eng.active_kernels["head"] and "weighted" in eng.active_kernels["seed"]
    rs, psi, res = eng.residual()
    assert close(psi.cpu().numpy(), fields["psi"], 5e-6, 2e-6)
    assert close(res.cpu().numpy(), fields["residual"], 2e-5, 1e-5)          # the residual field stays the plain r
    check_scalars(rs, osc)
    sc = eng.step()
    check_scalars(sc, osc)
    assert H.rel_err(eng.get_grad(), ograd) < 5e-5
    w = eng.weights()
    assert np.array_equal(bits(w["q"].cpu().numpy()), bits(c["q"]))
    assert abs(w["local"] - c["q"].sum(dtype=np.float64)) <= 1e-12 * w["local"] and w["total"] == w["local"]
    eng.close()


def test_zero_weight_rows_equal_the_batch_without_them_at_the_same_W():
    c = case("2d_plain", 37)
    keep = c["q"] > 0
    assert 0 < keep.sum() < 37
    osc, ograd, _ = weighted_loss_and_grad(c["pb"], c["flat"], c["x"][keep], c["q"][keep], W=float(c["q"].sum(dtype=np.float64)))
    eng = weighted_engine(c)
    eng.bind_weights(dev(c["q"]))
    sc = eng.step()
    check_scalars(sc, osc)
    assert H.rel_err(eng.get_grad(), ograd) < 5e-5
    eng.close()


# ---- 2. more points than one sweep of the head / seed grid --------------------------------------------------------------------------
def test_grid_stride_wrap_equals_the_duplicated_batch():
    """N = CUs * 1024 + 1025: every head workgroup takes a second round, the last two a ragged one.  Integer weights against an unweighted
    engine on the batch with row i repeated q_i times and n_global = sum q.  Both fp32 engines are held to the oracle bars of a step, so
    they may differ by twice those: gradient 1e-4, loss 2e-4, mu 4e-5."""
    N = torch.cuda.get_device_properties(0).multi_processor_count * 1024 + 1025
    kw = dict(layers=[2, 32, 32, 1], gamma=20.0)
    rng = np.random.default_rng(4)
    x = rng.uniform(-3, 3, (N, 2)).astype(np.float32)
    q = rng.integers(1, 4, N).astype(np.float32)
    flat = (rng.normal(0, 1, go.param_count(kw["layers"])) * 0.3).astype(np.float32)
    W = int(q.sum(dtype=np.float64))
    pb = go.Problem(**kw, dx=36.0 / W, w_bc=0.0)
    a = make_engine(pb, flat, x, None)
    a.bind_weights(dev(q))
    sa, ga = a.step(), a.get_grad()
    a.close()
    (xd,) = duplicated(x, q)
    b = make_engine(dataclasses.replace(pb, n_global=W), flat, xd, None)
    sb, gb = b.step(), b.get_grad()
    b.close()
    assert H.rel_err(ga, gb) < 1e-4
    assert abs(sa["loss"] - sb["loss"]) <= 2e-4 * abs(sb["loss"]) and abs(sa["mu"] - sb["mu"]) <= 4e-5 * abs(sb["mu"])
    for k in ("den", "sum_r2", "integral"):
        assert abs(sa[k] - sb[k]) <= 2e-4 * abs(sb[k]), k


# ---- 3. bound weights put the step on the standalone head / seed kernels --------------------------------------------------------------
@pytest.mark.parametrize("N", [4000, 40000])
def test_weights_route_the_step_to_the_standalone_head_and_seed_kernels(N):
    kw = dict(layers=[2, 64, 64, 64, 1], gamma=50.0, dx=36.0 / N)
    rng = np.random.default_rng(6)
    x = rng.uniform(-3, 3, (N, 2)).astype(np.float32)
    x_bc = rng.uniform(-3, 3, (5, 2)).astype(np.float32)
    flat = (rng.normal(0, 1, go.param_count(kw["layers"])) * 0.3).astype(np.float32)
    pb = go.Problem(**kw)
    a = make_engine(pb, flat, x, x_bc)
    k0 = a.active_kernels
    if "GPE_FUSE_HEAD" not in os.environ:
        assert ",head>" in k0["fwd"] and "head" not in k0, k0           # the default fuses the head at both sizes
    a.bind_weights(torch.ones(N, device="cuda"))
    k1 = a.active_kernels
    assert k1["head"].startswith("k_head_pde<") and k1["seed"].startswith("k_seed_pde<") and "weighted" in k1["head"] and "weighted" in k1["seed"]
    assert ",head>" not in k1["fwd"] and ",seeds" not in k1["bwd"], k1
    sa, ga = a.step(), a.get_grad()
    a.clear_weights()
    assert a.active_kernels == k0
    a.close()
    old = {k: os.environ.get(k) for k in ("GPE_FUSE_HEAD", "GPE_FUSE_SEED")}
    os.environ.update(GPE_FUSE_HEAD="0", GPE_FUSE_SEED="0")
    try:
        b = make_engine(pb, flat, x, x_bc)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    sb, gb = b.step(), b.get_grad()
    b.close()
    assert abs(sa["loss"] - sb["loss"]) <= 2e-6 * abs(sb["loss"])          # the bars of test_kernel_variants_agree
    assert H.rel_err(ga, gb) < 3e-6


# ---- 4. clearing restores the unweighted step ---------------------------------------------------------------------------------------
def test_clearing_weights_restores_the_old_step_bit_for_bit():
    """4 000 points of a plain real-psi problem: the default step there adds every sum in a fixed order (README, Reproducibility), so an
    engine that had weights bound and cleared must repeat, bit for bit, an engine that never had any."""
    N = 4000
    kw = dict(layers=[2, 64, 64, 64, 1], gamma=50.0, dx=36.0 / N)
    rng = np.random.default_rng(7)
    x = rng.uniform(-3, 3, (N, 2)).astype(np.float32)
    x_bc = rng.uniform(-3, 3, (5, 2)).astype(np.float32)
    flat = (rng.normal(0, 1, go.param_count(kw["layers"])) * 0.3).astype(np.float32)
    pb = go.Problem(**kw)
    out = []
    for with_weights in (True, False):
        e = make_engine(pb, flat, x, x_bc, sched=capi.SCHED_CONST)
        if with_weights:
            e.bind_weights(dev(weights_of(N)))
            e.clear_weights()
            with pytest.raises(GPEError):
                e.weights()
        scs = [e.step() for _ in range(5)]
        out.append((scs, e.get_params()))
        e.close()
    assert np.array_equal(bits(out[0][1]), bits(out[1][1]))
    assert out[0][0] == out[1][0]


# ---- 5. data parallel, both exchanges by hand -----------------------------------------------------------------------------------------
def test_data_parallel_by_hand_matches_the_weighted_reference():
    """three engines on the cuts (1, 17, N - 18) of N = 300 points, each with its rows of q and w_total = the global sum"""
    N = 300
    kw = dict(layers=[2, 64, 64, 64, 1], gamma=50.0)
    rng = np.random.default_rng(9)
    x = rng.uniform(-3, 3, (N, 2)).astype(np.float32)
    x_bc = rng.uniform(-3, 3, (5, 2)).astype(np.float32)
    flat = (rng.normal(0, 1, go.param_count(kw["layers"])) * 0.3).astype(np.float32)
    q = weights_of(N)
    W = float(q.sum(dtype=np.float64))
    pb = go.Problem(**kw, dx=float(np.float32(36.0 / W)))
    osc, ograd, _ = weighted_loss_and_grad(pb, flat, x, q, x_bc.astype(np.float64))
    cuts = H.dp_cuts(3, N)
    assert [hi - lo for lo, hi in cuts] == [1, 17, N - 18]
    engs = []
    try:
        for lo, hi in cuts:
            e = Engine(cfg_from_problem(pb, world_size=3))
            engs.append(e)
            e.set_params(flat)
            e.bind_points(dev(x[lo:hi]))
            e.bind_boundary(dev(x_bc))
            e.bind_weights(dev(q[lo:hi]), total=W)
            w = e.weights()
            assert w["total"] == W and abs(w["local"] - q[lo:hi].sum(dtype=np.float64)) <= 1e-12 * W
        dp_step(engs)
        scs = [e.read_scalars() for e in engs]
        check_scalars(scs[0], osc)
        assert H.rel_err(engs[0].get_grad(), ograd) < 5e-5
        p0 = engs[0].get_params()
        for r in (1, 2):
            assert scs[r]["loss"] == scs[0]["loss"] and scs[r]["mu"] == scs[0]["mu"]
            assert np.array_equal(bits(engs[r].get_params()), bits(p0))
    finally:
        for e in engs:
            e.close()


# ---- 6. graded stratified sampler -----------------------------------------------------------------------------------------------------
EDGES = {1: [S.sinh_edges(6.0, 257, 2.0)], 2: [S.sinh_edges(4.0, 17, 2.5), S.sinh_edges(3.0, 19, 1.0)],
         3: [S.sinh_edges(4.0, 5, 1.5), S.sinh_edges(3.0, 7, 2.0), S.sinh_edges(2.0, 9, 0.5)]}
GRADED_NET = {1: [1, 32, 32, 1], 2: [2, 64, 64, 64, 1], 3: [3, 64, 64, 1]}


def graded_engine(d, seed=0, **cfg):
    kw = dict(layers=GRADED_NET[d], gamma=20.0, dx=1.0, w_bc=0.0)
    kw.update(cfg)
    pb = go.Problem(**kw)
    flat = (np.random.default_rng(21 + seed).normal(0, 1, go.param_count(kw["layers"])) * 0.3).astype(np.float32)
    eng = Engine(cfg_from_problem(pb, sched=capi.SCHED_CONST))
    eng.set_params(flat)
    return eng, pb, flat


@pytest.mark.parametrize("d", [1, 2, 3])
def test_graded_sampler_holds_the_numpy_restatement_bit_for_bit(d):
    ed = EDGES[d]
    total = int(np.prod([a.size - 1 for a in ed]))
    eng, _, _ = graded_engine(d)
    eng.bind_sampler_graded(ed, every=1, seed=77, draw0=5)
    pts, draw = eng.sampler_points()
    w = eng.weights()
    assert draw == 5 and pts.shape == (total, d)
    assert np.array_equal(bits(pts.cpu().numpy()), bits(S.graded_points(ed, 77, 5)))
    q = S.graded_weights(ed)
    assert np.array_equal(bits(w["q"].cpu().numpy()), bits(q))
    assert w["total"] == S.graded_total(ed)
    assert abs(w["local"] - q.sum(dtype=np.float64)) <= 1e-12 * w["total"]
    assert "weighted" in eng.active_kernels["head"]
    # two engines holding halves hold the set of one, and report the whole grid's W
    h = total // 2 + 1
    for first, n in ((0, h), (h, total - h)):
        e2, _, _ = graded_engine(d)
        e2.bind_sampler_graded(ed, every=1, seed=77, draw0=5, first_cell=first, n=n)
        p2, w2 = e2.sampler_points()[0], e2.weights()
        assert np.array_equal(bits(p2.cpu().numpy()), bits(pts.cpu().numpy()[first:first + n]))
        assert np.array_equal(bits(w2["q"].cpu().numpy()), bits(q[first:first + n]))
        assert w2["total"] == w["total"] and abs(w2["local"] - q[first:first + n].sum(dtype=np.float64)) <= 1e-12 * w["total"]
        e2.close()
    # a redraw changes the points and not the weights
    eng.step(); eng.step()
    pts1, draw1 = eng.sampler_points()
    assert draw1 == 6 and np.array_equal(bits(pts1.cpu().numpy()), bits(S.graded_points(ed, 77, 6))) and not torch.equal(pts1, pts)
    assert np.array_equal(bits(eng.weights()["q"].cpu().numpy()), bits(q))
    eng.close()


def test_step_behind_a_redraw_matches_the_weighted_reference():
    ed = EDGES[2]
    eng, pb, _ = graded_engine(2)
    eng.bind_sampler_graded(ed, every=1, seed=5)
    eng.step()
    flat1 = eng.get_params()
    sc = eng.step()                               # redraws to draw 1, then steps on it
    pts, draw = eng.sampler_points()
    assert draw == 1
    w = eng.weights()
    osc, ograd, _ = weighted_loss_and_grad(pb, flat1, pts.cpu().numpy(), w["q"].cpu().numpy(), W=w["total"])
    check_scalars(sc, osc)
    assert H.rel_err(eng.get_grad(), ograd) < 5e-5
    eng.close()


def test_graded_trajectory_equals_host_loop_of_bind_points_and_bind_weights():
    """12 steps of run() with every = 5 == bind_points(graded_points(draw m)) + bind_weights(graded_weights, graded_total) + run per chunk:
    parameters and Adam moments bit for bit (323 points: one head workgroup, so every sum is added in a fixed order)."""
    ed = EDGES[2]
    a, _, _ = graded_engine(2)
    a.bind_sampler_graded(ed, every=5, seed=31337)
    a.run(12)
    b, _, _ = graded_engine(2)
    for m, k in enumerate((5, 5, 2)):
        b.bind_points(dev(S.graded_points(ed, 31337, m)))
        b.bind_weights(dev(S.graded_weights(ed)), total=S.graded_total(ed))
        b.run(k)
    sa = (a.get_params(),) + a.get_adam_state()
    sb = (b.get_params(),) + b.get_adam_state()
    assert sa[3] == sb[3] == 12
    for p, r in zip(sa[:3], sb[:3]):
        assert np.array_equal(bits(p), bits(r))
    assert a.sampler_points()[1] == 2
    a.close(); b.close()


def test_frozen_orthogonality_state_is_refilled_behind_a_graded_redraw():
    ed = EDGES[1]
    kw = dict(layers=GRADED_NET[1], gamma=20.0, dx=1.0, w_bc=0.0, w_orth=2.0)
    eng, _, _ = graded_engine(1, w_orth=2.0)
    theta = _frozen(kw, 1)
    eng.bind_orth_state(0, theta)
    eng.bind_sampler_graded(ed, every=1, seed=3)
    psi0 = eng.orth_values(0).cpu().numpy()
    eng.step(); eng.step()
    pts, draw = eng.sampler_points()
    psi1 = eng.orth_values(0).cpu().numpy()
    assert draw == 1 and not np.array_equal(psi0, psi1)
    want = _oracle_psi(kw, theta, pts.cpu().numpy())
    assert close(psi1, want, 1e-5, 2e-6)
    eng.close()


# ---- 7. observables on the bound set --------------------------------------------------------------------------------------------------
OBS_FIELDS = ("norm", "kin", "pot", "inter", "rot", "energy", "mu", "mu_lap", "lz", "res_rms")


@pytest.mark.parametrize("name", ["2d_plain", "2d_complex_rot_128"])
def test_observables_with_integer_weights_equal_the_duplicated_set(name):
    """fp64 sums of the same fp32 jets, only the order differs: 1e-10 relative (moments: of the box scale, they cancel around 0)"""
    c = case(name, 1025)
    q = np.random.default_rng(12).integers(1, 4, 1025).astype(np.float32)
    a = weighted_engine(c)
    a.bind_weights(dev(q))
    oa = a.observables(dv=0.01)
    a.close()
    (xd,) = duplicated(c["x"], q)
    b = make_engine(c["pb"], c["flat"], xd, None, path=PATHS["fused"])
    ob = b.observables(dv=0.01)
    b.close()
    assert oa["n"] == 1025 and ob["n"] == q.sum()
    for k in OBS_FIELDS:
        assert abs(oa[k] - ob[k]) <= 1e-10 * abs(ob[k]), (k, oa[k], ob[k])
    for k in range(2):
        assert abs(oa["mean_x"][k] - ob["mean_x"][k]) <= 1e-10 * 3.0 and abs(oa["var_x"][k] - ob["var_x"][k]) <= 1e-10 * 9.0
    assert abs(oa["peak_density"] - ob["peak_density"]) <= 1e-10 * ob["peak_density"]


def test_observables_with_real_weights_equal_fp64_host_sums_over_the_engines_own_jets():
    c = case("2d_plain", 1025)
    pb, x, q = c["pb"], c["x"], c["q"].astype(np.float64)
    eng = weighted_engine(c)
    J = eng.forward_jets(dev(x)).cpu().numpy().astype(np.float64)
    eng.bind_weights(dev(c["q"]))
    got = eng.observables(dv=0.01)
    plain = eng.observables(dev(x), dv=0.01)          # an explicit set stays unweighted, even the bound one
    eng.close()
    u = J[0, :, 0]
    rho = u * u
    sr, dv, tol = (q * rho).sum(), float(np.float32(0.01)), 1e-9
    I = dv * sr
    assert got["n"] == 1025
    assert abs(got["norm"] - I) <= tol * I
    kin = float(np.float32(pb.kinetic_coeff)) * (q * (J[1:3, :, 0] ** 2).sum(0)).sum() / sr
    assert abs(got["kin"] - kin) <= tol * kin
    s = float(np.float32(pb.gamma)) * u ** (pb.p + 1)
    inter = 2.0 / (pb.p + 1) * dv * (q * s).sum() / I ** (0.5 * (pb.p + 1))
    assert abs(got["inter"] - inter) <= tol * inter
    x64 = x.astype(np.float64)
    for k in range(2):
        m1, m2 = (q * x64[:, k] * rho).sum() / sr, (q * x64[:, k] ** 2 * rho).sum() / sr
        assert abs(got["mean_x"][k] - m1) <= tol * (q * np.abs(x64[:, k]) * rho).sum() / sr
        assert abs(got["var_x"][k] - (m2 - m1 * m1)) <= 4 * tol * m2
    assert abs(got["peak_density"] - rho.max() / I) <= tol * rho.max() / I          # the plain maximum
    assert abs(plain["norm"] - dv * rho.sum()) <= tol * dv * rho.sum()


# ---- 8. refusals and lifetime ---------------------------------------------------------------------------------------------------------
def _code(fn, *a, **k):
    with pytest.raises(GPEError) as ex:
        fn(*a, **k)
    return ex.value.code


def test_refusals_and_lifetime():
    c = case("2d_plain", 37)
    N, q = 37, c["q"]
    eng = Engine(cfg_from_problem(c["pb"]))
    eng.set_params(c["flat"])
    eng.n_local = N
    assert _code(eng.bind_weights, dev(q)) == capi.GPE_ERR_STATE                   # no points bound
    assert _code(eng.weights) == capi.GPE_ERR_STATE
    eng.bind_points(dev(c["x"]))
    for bad in (-1.0, np.nan, np.inf):
        b = q.copy(); b[5] = bad
        assert _code(eng.bind_weights, dev(b)) == capi.GPE_ERR_INVALID
    assert _code(eng.bind_weights, dev(np.zeros(N))) == capi.GPE_ERR_INVALID      # w_local == 0
    for bad in (-1.0, float("nan"), float("inf")):
        assert _code(eng.bind_weights, dev(q), total=bad) == capi.GPE_ERR_INVALID
    assert _code(eng.weights) == capi.GPE_ERR_STATE                               # nothing got bound on the way
    eng.bind_weights(dev(q), total=100.0)
    assert eng.weights()["total"] == 100.0
    b = q.copy(); b[0] = -2.0
    assert _code(eng.bind_weights, dev(b)) == capi.GPE_ERR_INVALID                # a failed bind leaves the previous weights
    w = eng.weights()
    assert w["total"] == 100.0 and np.array_equal(bits(w["q"].cpu().numpy()), bits(q))
    assert _code(eng.set_n_global, 50) == capi.GPE_ERR_STATE
    assert _code(eng.set_loss_weights, 1.0, 0.0, 20.0, w_sym=5.0) == capi.GPE_ERR_INVALID
    eng.clear_weights()
    eng.set_n_global(50)                                                          # works again
    eng.set_n_global(0)
    eng.bind_weights(dev(q))
    eng.bind_points(dev(c["x"]))                                                  # a bind of points clears them
    assert _code(eng.weights) == capi.GPE_ERR_STATE
    eng.bind_weights(dev(q))
    eng.bind_sampler((-3, -3), (3, 3), (6, 6), every=4)                           # ... and so does a bind of the sampler
    assert _code(eng.weights) == capi.GPE_ERR_STATE
    eng.n_local = 36
    assert _code(eng.bind_weights, dev(q[:36])) == capi.GPE_ERR_STATE             # a sampler is bound: its rows move
    ed = [S.sinh_edges(3.0, 6, 1.0)] * 2
    eng.bind_sampler_graded(ed, every=4)
    assert _code(eng.bind_weights, dev(q[:36])) == capi.GPE_ERR_STATE
    assert _code(eng.clear_weights) == capi.GPE_ERR_STATE                         # the graded sampler owns its weights
    assert _code(eng.set_n_global, 50) == capi.GPE_ERR_STATE
    # graded binds the engine refuses: edges that do not increase / are not finite, lo / hi other than the end edges
    flat_edge = ed[0].copy(); flat_edge[3] = flat_edge[2]
    nan_edge = ed[0].copy(); nan_edge[2] = np.nan
    sp = capi.gpe_sampler_spec()
    for k in range(2):
        sp.shape[k], sp.lo[k], sp.hi[k], sp.clip_lo[k], sp.clip_hi[k] = 6, -3.0, 3.0, -3.0, 3.0
    sp.n_local, sp.every = 36, 4
    import ctypes as C
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda s, e0, e1: eng.lib.gpe_bind_sampler_graded(eng._h, C.byref(s), e0, e1, None)
    assert call(sp, ptr(flat_edge), ptr(ed[1])) == capi.GPE_ERR_INVALID
    assert call(sp, ptr(nan_edge), ptr(ed[1])) == capi.GPE_ERR_INVALID
    assert call(sp, ptr(ed[0]), None) == capi.GPE_ERR_INVALID
    sp.lo[0] = -2.5
    assert call(sp, ptr(ed[0]), ptr(ed[1])) == capi.GPE_ERR_INVALID
    sp.lo[0], sp.every = -3.0, 0
    assert call(sp, ptr(ed[0]), ptr(ed[1])) == capi.GPE_ERR_INVALID
    assert eng.weights()["total"] == S.graded_total(ed)                           # the refused binds left the graded sampler in place
    eng.clear_sampler()                                                           # clears it, weights included
    assert _code(eng.weights) == capi.GPE_ERR_STATE
    eng.close()
    # the symmetry batch has no weights
    sym = Engine(cfg_from_problem(dataclasses.replace(c["pb"], w_sym=5.0)))
    sym.set_params(c["flat"])
    sym.bind_points(dev(c["x"]))
    assert _code(sym.bind_weights, dev(q)) == capi.GPE_ERR_INVALID
    with pytest.raises(GPEError) as ex:
        sym.bind_sampler_graded(ed, every=4)
    assert ex.value.code == capi.GPE_ERR_INVALID
    sym.close()
