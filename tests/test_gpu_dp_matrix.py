"""Data-parallel step at world 3 and 8 against the fp64 oracle, per loss flavour and network class.

A cell = (case, kernel set, world): W engines on one GPU, each created with world_size = W and n_global = N and bound to its contiguous
block of the points (with its rows of every per-point array: potential, precomputed base, orthogonality arrays) and to the whole
boundary batch.  The two exchanges of a step are done by hand -- exchange_sums and exchange_grad summed in float64 in rank order and
copied back to every engine -- which is what the all-reduces do.  The cuts are explicit (tests/helpers.py: dp_cuts): 1-point shards,
shards one below, at and one above the 16-point tile, and ranks whose boundary batch rides in the collocation launch next to ranks where
it does not.

The reference is go.full_loss_and_grad on all N points in float64; the bounds are those of test_step_matches_oracle (mu 2e-5, loss
pieces 1e-4, norm 2e-4, gradient 5e-5 of max|g|), the gradient also per weight matrix and bias at 5e-5 of that block's own maximum.
That the per-block bound can be met in fp32 is shown by the oracle itself run on float32 inputs (< 1e-5 per block, CPU side).

Cases whose CASES entry has fewer than 333 points run at 400 (the world-8 cut needs 315); entries above 777 points run at 777."""
import dataclasses
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from gpe_pinn import Engine
from oracle import gpe_oracle as go
from tests import helpers as H
from tests.test_gpu_orth_states import _frozen, _oracle_psi
from tests.test_gpu_parity import CASES, ORTH_CASES, PATHS, _inputs, _orth_modes, _scale, cfg_from_problem

pytestmark = pytest.mark.gpu

WORLDS = (3, 8)
N_FLOOR, N_SMALL, N_CAP = 333, 400, 777

MATRIX = ["2d_64x4_g500", "1d_64x4_m3_p4_odd", "1d_32x4_nb_sym", "2d_complex_rot_variational", "2d_128x6_complex_cfg4", "2d_class_loss_64x4",
          "3d_energy_lambda_p5_256x2", "2d_128x5_cfg3", "2d_riesz_variational", "1d_reg_f_rayleigh", "1d_residual_64x2blocks",
          "2d_residual_128x3blocks", "1d_single_hidden", "2d_100x3_reference_2d_arch"]
# per-point arrays of the caller, cut by rows: orthogonality arrays, frozen states (each rank fills its own rows), the gravity well
# (precomputed potential and Airy base, boundary target folded in)
EXTRA = ["orth_caller_arrays", "orth_frozen_states", "gravity_well"]
THREE_STEPS = {"2d_64x4_g500", "1d_64x4_m3_p4_odd", "2d_complex_rot_variational"}
SCALAR_TOLS = (("mu", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("bc", 1e-4), ("norm", 2e-4), ("sym", 1e-4), ("orth", 1e-4), ("riesz", 1e-4),
               ("reg", 1e-4))

_SETUP = {}


def _setup(name):
    """the problem, its inputs on all N points and (filled by _oracle) its reference, built once per module run and left unchanged"""
    if name in _SETUP:
        return _SETUP[name]
    s = dict(bc_target=None, V=None, base=None, orth=None, states=(), fused_ok=True)
    if name in CASES:
        kw, n_case, s["fused_ok"] = CASES[name]
        N = N_SMALL if n_case < N_FLOOR else min(n_case, N_CAP)
        x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
        pb = go.Problem(**kw, n_global=N)
    elif name == "orth_caller_arrays":
        kw, N, n_o = ORTH_CASES["2d_128_two_modes"]
        x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
        pb = go.Problem(**kw, n_global=N)
        s["orth"] = _orth_modes(x, n_o)
    elif name == "orth_frozen_states":
        kw, N = ORTH_CASES["1d_two_modes"][0], N_CAP
        x, flat, x_bc = _inputs(kw, N, scale=_scale(kw))
        pb = go.Problem(**kw, n_global=N)
        s["states"] = ((_frozen(kw, 1), 0, 0.37, 1.0), (_frozen(kw, 2), 1, 0.5, 0.8))          # (parameters, base mode, perturb scale, amplitude)
        s["orth"] = np.stack([_oracle_psi(kw, th, x, bm, ps, amp) for th, bm, ps, amp in s["states"]])
    elif name == "gravity_well":
        fx = H.load_fx("fx_vbeta_gravity_m0_b0.5_g0.npz")
        pb, arr = H.problem_from_vbeta(fx)
        x, flat = fx["x"].astype(np.float32), fx["flat0"].astype(np.float32)
        N = x.shape[0]
        pb = dataclasses.replace(pb, n_global=N)
        x_bc = np.array([[float(fx["lb"])], [float(fx["ub"])]], np.float32)
        s.update(V=np.asarray(arr["V_pre"], np.float64), base=tuple(np.asarray(a, np.float64) for a in arr["base_pre"]),
                 bc_target=np.asarray(arr["bc_target"], np.float64))
    else:
        raise KeyError(name)
    assert N_FLOOR <= N <= N_CAP
    s.update(pb=pb, N=N, x=x, flat=flat, x_bc=x_bc, blocks=H.param_blocks(pb.layers, pb.net_kind))
    _SETUP[name] = s
    return s


def _oracle_args(s, dt):
    c = lambda a: None if a is None else np.asarray(a, dt)
    return dict(x_bc=c(s["x_bc"]), bc_target=c(s["bc_target"]), V_pre=c(s["V"]), orth=c(s["orth"]),
                base_pre=None if s["base"] is None else tuple(c(a) for a in s["base"]))


def _oracle(name, steps=1):
    s = _setup(name)
    pb, flat, x = s["pb"], s["flat"], s["x"]
    if "osc" not in s:
        osc, ograd, _ = go.full_loss_and_grad(pb, flat.astype(np.float64), x.astype(np.float64), **_oracle_args(s, np.float64))
        _, g32, _ = go.full_loss_and_grad(pb, flat, x, **_oracle_args(s, np.float32))          # the same call in float32
        new, _, _ = go.optimizer_step(go.OptState(lr0=1e-3), flat, ograd, osc["loss"])
        s.update(osc=osc, ograd=ograd, new=new, f32_blocks=H.block_rel_errs(g32, ograd, s["blocks"]))
    if steps > 1 and "traj" not in s:
        _, tr = go.train_steps(pb, go.OptState(lr0=1e-3), flat.astype(np.float64), x.astype(np.float64), steps, dtype=np.float64,
                               **_oracle_args(s, np.float64))
        s["traj"] = np.array([t["loss"] for t in tr])
    return s


@contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def make_rank(s, path, world, lo, hi):
    """the engine of one rank: world_size = world, n_global = N, rows lo..hi of the points and of every per-point array, the whole boundary batch"""
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")
    eng = Engine(cfg_from_problem(s["pb"], path=PATHS[path], world_size=world))
    try:
        eng.set_params(s["flat"])
        eng.bind_points(dev(s["x"][lo:hi]), V=None if s["V"] is None else dev(s["V"][lo:hi]))
        if s["base"] is not None:
            eng.bind_base(*[dev(a[lo:hi]) for a in s["base"]])
        eng.bind_boundary(dev(s["x_bc"]), None if s["bc_target"] is None else dev(s["bc_target"]))
        if s["states"]:
            for j, (th, bm, ps, amp) in enumerate(s["states"]):
                eng.bind_orth_state(j, th, base_mode=bm, perturb_scale=ps, amplitude=amp)
        elif s["orth"] is not None:
            for j in range(s["orth"].shape[0]):
                eng.bind_orth(j, dev(s["orth"][j, lo:hi]))
    except Exception:
        eng.close()
        raise
    return eng


def dp_step(engs):
    """one data-parallel step of the engines of all ranks: the three phases with both sum-exchanges done by hand, in float64, in rank order"""
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


def check_rank0(sc, grad, params, s):
    """failures of rank 0's scalars, gradient (whole and per parameter block) and updated parameters against the fp64 oracle"""
    bad = []
    osc, ograd = s["osc"], s["ograd"]
    for k, tol in SCALAR_TOLS:
        if not abs(sc[k] - osc[k]) <= tol * max(abs(osc[k]), 1e-6):
            bad.append(f"{k} {sc[k]:.9g} vs oracle {osc[k]:.9g}")
    gn = float(np.linalg.norm(ograd))
    if not abs(sc["grad_norm"] - gn) < 1e-4 * gn:
        bad.append(f"grad_norm {sc['grad_norm']:.9g} vs oracle {gn:.9g}")
    eg = H.rel_err(grad, ograd)
    if not eg < 5e-5:
        bad.append(f"gradient rel err {eg:.3e}")
    for nm, e in H.block_rel_errs(grad, ograd, s["blocks"]).items():
        if not e < 5e-5:
            bad.append(f"gradient block {nm}: {e:.3e} of its own maximum (float32 oracle: {s['f32_blocks'][nm]:.3e})")
    d = np.abs(params - s["new"])
    if not (np.quantile(d, 0.99) < 2e-5 and d.max() < 2.1e-3):
        bad.append(f"parameters after Adam: q99 {np.quantile(d, 0.99):.3e} max {d.max():.3e}")
    return bad


def run_cell(name, path, world, env=None):
    steps = 3 if name in THREE_STEPS else 1
    s = _oracle(name, steps)
    worst = max(s["f32_blocks"].values())
    cuts = H.dp_cuts(world, s["N"])
    assert cuts[0][0] == 0 and cuts[-1][1] == s["N"] and all(cuts[r][1] == cuts[r + 1][0] for r in range(world - 1))
    engs, bad = [], []
    with _environment(env or {}):
        try:
            for lo, hi in cuts:
                try:
                    engs.append(make_rank(s, path, world, lo, hi))
                except ValueError as ex:          # gpe_create: GPE_ERR_INVALID -- the only reason a cell may skip, and never on the generic set
                    if path == "generic":
                        raise
                    pytest.skip(f"gpe_create refuses the fused path for this network: {ex}")
                assert engs[-1].active_path == PATHS[path]
            kernels = [e.active_kernels for e in engs]
            losses = []
            for k in range(steps):
                dp_step(engs)
                scs = [e.read_scalars() for e in engs]
                params = [e.get_params() for e in engs]
                losses.append(scs[0]["loss"])
                for r in range(1, world):
                    if scs[r]["mu"] != scs[0]["mu"] or scs[r]["loss"] != scs[0]["loss"]:
                        bad.append(f"step {k}: rank {r} reports mu {scs[r]['mu']!r} loss {scs[r]['loss']!r}, rank 0 mu {scs[0]['mu']!r} loss {scs[0]['loss']!r}")
                    if not np.array_equal(params[r], params[0]):
                        bad.append(f"step {k}: parameters of rank {r} differ from rank 0's (max {np.abs(params[r] - params[0]).max():.3e})")
                if k == 0:
                    grad = engs[0].get_grad()
                    blk = H.block_rel_errs(grad, s["ograd"], s["blocks"])
                    print(f"[{name}-{path}-w{world}] N {s['N']} mu {abs(scs[0]['mu'] - s['osc']['mu']) / max(abs(s['osc']['mu']), 1e-6):.2e} "
                          f"loss {abs(scs[0]['loss'] - s['osc']['loss']) / abs(s['osc']['loss']):.2e} grad {H.rel_err(grad, s['ograd']):.2e} "
                          f"worst block {max(blk, key=blk.get)} {max(blk.values()):.2e} (float32 oracle worst {worst:.2e})")
                    bad += check_rank0(scs[0], grad, params[0], s)
            if steps > 1:
                dev = max(abs(a - t) / max(abs(t), 1e-30) / (1 + k) for k, (a, t) in enumerate(zip(losses, s["traj"])))
                print(f"[{name}-{path}-w{world}] {steps}-step loss trajectory off the oracle's by {dev:.2e}")
                if not dev < 1e-3:
                    bad.append(f"{steps}-step loss trajectory off the oracle's: {dev:.3e} ({losses} vs {s['traj'].tolist()})")
        finally:
            for e in engs:
                e.close()
    assert not bad, f"{name} {path} world {world}: {len(bad)} failing checks\n" + "\n".join(bad[:40])
    return kernels


def _cells():
    out = []
    for name in MATRIX + EXTRA:
        fused_ok = CASES[name][2] if name in CASES else True
        for path in ("generic", "fused") if fused_ok else ("generic",):
            for world in WORLDS:
                out.append(pytest.param(name, path, world, id=f"{name}-{path}-w{world}"))
    return out


@pytest.mark.parametrize("name,path,world", _cells())
def test_dp_step_matches_oracle(name, path, world):
    run_cell(name, path, world)


@pytest.mark.parametrize("name", MATRIX + EXTRA)
def test_float32_oracle_reaches_the_per_block_bound(name):
    """CPU side: the oracle's own call on float32 inputs stays below 1e-5 of every parameter block's maximum against its float64 self, so
    the 5e-5 asked of the engine per block is within reach of fp32 arithmetic.

    This check found the one sum of the oracle that did not accumulate in float64: mlp_backward's dW / db over the points.  np.einsum
    adds its C*N float32 terms one after the other, and 3d_energy_lambda_p5_256x2 at its 400 points lost 1.5e-5 on the output map's
    weights to that (2d_riesz_variational 1.2e-5 at 900 points; the other cases 6.6e-7 .. 9.5e-6, growing with N), while the engine held
    1.0e-6.  With dW / db accumulated in float64 like the oracle's other sums -- bit for bit the same for float64 inputs -- the float32
    call gives, worst block per case: 3d_energy_lambda_p5_256x2 5.5e-7, 2d_100x3_reference_2d_arch 8.5e-7, 1d_residual_64x2blocks 6.6e-7,
    every other case between 7.9e-8 and 4.7e-7."""
    s = _oracle(name)
    worst = max(s["f32_blocks"], key=s["f32_blocks"].get)
    print(f"[{name}] N {s['N']} float32 oracle worst block {worst} {s['f32_blocks'][worst]:.2e}")
    assert s["f32_blocks"][worst] < 1e-5, s["f32_blocks"]


@pytest.mark.parametrize("world", WORLDS)
def test_dp_step_matches_oracle_on_the_per_wave_tile_kernels(world):
    """GPE_COOP=0 (set before the engines are created and held for their life): the per-wave-tile forward / reverse pair through the
    three phases instead of the cooperative whole-network kernels"""
    s = _setup("2d_64x4_g500")
    lo, hi = H.dp_cuts(world, s["N"])[-1]
    eng = make_rank(s, "fused", world, lo, hi)
    default = eng.active_kernels
    eng.close()
    kernels = run_cell("2d_64x4_g500", "fused", world, env={"GPE_COOP": "0"})
    assert (kernels[-1]["fwd"], kernels[-1]["bwd"]) != (default["fwd"], default["bwd"]), (kernels[-1], default)
