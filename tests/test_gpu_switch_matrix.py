"""Switch matrix: every documented kernel-selection switch (tests/switch_table.py) against the fp64 oracle, for every network class the
switch applies to.  A cell = (class, batch, switch value): the engine is created under that environment (held for its whole life: some
switches are read at launch), and forward_jets, residual(), one step (mu and every loss term), the gradient and the parameters after
Adam are held to the tolerances of test_step_matches_oracle.  Rows that promise bit-identical results are also compared with the
default engine bit for bit, and rows of execution modes follow a 9-step trajectory of the oracle's optimiser.

Large-batch kernels are reached at sizes the oracle can do through the threshold switches (stand-ins); the stand-in must report the
same active_kernels string as the default engine at the real size (test_large_batch_stand_ins_report_the_kernels_of_the_real_size)."""
import json
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import Engine
from oracle import gpe_oracle as go
from tests import helpers as Hl
from tests import switch_table as T
from tests.test_gpu_parity import cfg_from_problem, close

pytestmark = pytest.mark.gpu

ANISO = (1.0, 1.4, 2.0)
# stand-in for the headline large batch at H <= 64 (per-wave-tile forward with the head inside, f_backward_pipe without seeds,
# uneven tile split in both): the same kernels and split as the default engine at 540 000 points
LARGE64 = {"GPE_COOP_FWD_MAX_TILES": "0", "GPE_FUSE_HEAD_TILE_MIN": "0", "GPE_SHARE_MIN_TILES": "1", "GPE_FUSE_SEED_MAX": "0"}
# H = 128 in 1D / 2D: the wide set's per-map reverse kernels, taken by default from 2 048 tiles on
LARGE128 = {"GPE_WIDE_MIN_TILES": "0"}

# name: (Problem kwargs, [(N, base environment, real size the base environment stands in for)], path, descriptor overrides, orth modes)
CLASSES = {
    "1d_h32_2maps_hermite": (dict(layers=[1, 32, 32, 32, 1], gamma=5.0, base_mode=0, dx=12 / 332), [(333, {}, None), (16, {}, None)],
                             None, {}, 0),
    "ns_2d_64x4_g500": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=500.0, dx=36 / 777), [(777, {}, None), (40001, LARGE64, 540000)],
                        None, {}, 0),
    "2d_64_5maps": (dict(layers=[2, 64, 64, 64, 64, 64, 64, 1], gamma=20.0, dx=0.01), [(401, {}, None)], None, {}, 0),
    "3d_64x3": (dict(layers=[3, 64, 64, 64, 1], gamma=20.0, dx=0.01, omega=ANISO), [(130, {}, None)], None, {}, 0),
    "res1_1d_64": (dict(layers=[1, 64, 64, 1], net_kind=go.NET_RESIDUAL, activation=1, kinetic_coeff=1.0, gamma=2.0, base_mode=0,
                        perturb_scale=0.05, dx=0.03), [(200, {}, None)], None, {}, 0),
    "res2_2d_32": (dict(layers=[2, 32, 32, 32, 1], net_kind=go.NET_RESIDUAL, gamma=5.0, dx=0.01), [(300, {}, None)], None, {}, 0),
    "complex_2d_64": (dict(layers=[2, 64, 64, 64, 2], complex_psi=True, gamma=30.0, omega_rot=0.8, dx=0.02), [(200, {}, None)], None, {}, 0),
    "cfg4_2d_128x5maps_complex": (dict(layers=[2, 128, 128, 128, 128, 128, 128, 2], complex_psi=True, gamma=50.0, omega_rot=0.8, dx=0.01),
                                  [(150, {}, None), (150, LARGE128, 262144)], None, {}, 0),
    "cfg3_2d_128x4maps": (dict(layers=[2, 128, 128, 128, 128, 128, 1], gamma=500.0, dx=0.01), [(200, {}, None), (200, LARGE128, 131072)],
                          None, {}, 0),
    "3d_128x3": (dict(layers=[3, 128, 128, 128, 1], gamma=100.0, dx=0.001, omega=ANISO), [(130, {}, None)], None, {}, 0),
    "3d_256x3": (dict(layers=[3, 256, 256, 256, 1], gamma=100.0, dx=0.01, omega=ANISO), [(100, {}, None)], None, {}, 0),
    "orth_1d_64": (dict(layers=[1, 64, 64, 64, 1], gamma=3.0, base_mode=2, w_orth=7.0, dx=12 / 299), [(300, {}, None)], None,
                   {"loss": "orth"}, 2),
    "sym_1d_32x3": (dict(layers=[1, 32, 32, 32, 32, 1], gamma=1.0, base_mode=0, base_deriv=1, w_sym=5.0, dx=12 / 299), [(300, {}, None)],
                    None, {"loss": "sym"}, 0),
    "riesz_2d_64": (dict(layers=[2, 64, 64, 64, 1], gamma=100.0, kinetic_coeff=1.0, pot_scale=1.0, w_riesz=0.05, riesz_kind=go.RIESZ_SUM,
                         dx=36 / 400), [(400, {}, None)], None, {"loss": "riesz"}, 0),
    "energy_2d_64": (dict(layers=[2, 64, 64, 64, 64, 1], gamma=100.0, kinetic_coeff=1.0, pot_scale=1.0, w_norm=0.0, lambda_kind=go.LAMBDA_ENERGY,
                          w_reg_f=1.0, w_reg_lam=1.0, dx=1.0), [(500, {}, None)], None, {"loss": "energy"}, 0),
    "pad48_2d": (dict(layers=[2, 48, 48, 48, 1], gamma=10.0, dx=0.01), [(300, {}, None)], None, {"H": 64, "pad": True}, 0),
    "pad100_2d": (dict(layers=[2, 100, 100, 100, 1], gamma=100.0, kinetic_coeff=1.0, pot_scale=1.0, dx=0.01), [(500, {}, None)], None,
                  {"H": 128, "pad": True}, 0),
    # generic set: residual blocks of 64 beyond two (g_fwd_layer_mfma), of width 48 (g_fwd_layer), width 512 (g_fwd_layer_mfma2)
    "gen_res3_64": (dict(layers=[1, 64, 64, 64, 64, 1], net_kind=go.NET_RESIDUAL, activation=1, kinetic_coeff=1.0, potential=go.POT_GAUSSIAN,
                         pot_a=0.5, gamma=3.0, p=4, base_mode=1, perturb_scale=0.05, dx=0.03), [(333, {}, None)], None, {"path": "generic"}, 0),
    "gen_res1_48": (dict(layers=[2, 48, 48, 1], net_kind=go.NET_RESIDUAL, gamma=5.0, dx=0.01), [(200, {}, None)], None, {"path": "generic"}, 0),
    "gen_2d_512": (dict(layers=[2, 512, 512, 1], gamma=10.0, dx=0.01), [(64, {}, None)], None, {"path": "generic"}, 0),
}


def descriptor(name, bi):
    kw, batches, _, over, _ = CLASSES[name]
    layers = kw["layers"]
    res = kw.get("net_kind", go.NET_MLP) == go.NET_RESIDUAL
    hid = layers[1:-1]
    H = max(hid)
    maps = 2 * (len(layers) - 3) if res else len(hid) - 1
    loss = "plain"
    d = dict(H=H, maps=maps, res=res, n_out=layers[-1], dim=layers[0], loss=loss, pad=False, large=batches[bi][2] is not None)
    d.update(over)
    if "path" not in d:
        d["path"] = "wide" if d["H"] >= 128 else "fused"
    run_layers = [layers[0]] + [d["H"]] * len(hid) + [layers[-1]]
    d["P"] = go.param_count(run_layers, kw.get("net_kind", go.NET_MLP))
    assert set(d) == set(T.CLASS_KEYS)
    return d


CELLS = [(name, bi) for name in CLASSES for bi in range(len(CLASSES[name][1]))]


def _scale(layers):
    w = max(layers[1:-1])
    return 0.3 if w <= 64 else (0.15 if w <= 128 else (0.1 if w <= 256 else 0.06))


_INPUTS = {}


def inputs(name, N):
    key = (name, N)
    if key not in _INPUTS:
        kw = CLASSES[name][0]
        layers = kw["layers"]
        rng = np.random.default_rng(N)
        d = layers[0]
        x = (np.linspace(-6, 6, N).reshape(-1, 1) if d == 1 else rng.uniform(-3, 3, (N, d))).astype(np.float32)
        flat = (rng.normal(0, 1, go.param_count(layers, kw.get("net_kind", 0))) * _scale(layers)).astype(np.float32)
        x_bc = (np.array([[-6.0], [6.0]]) if d == 1 else rng.uniform(-3, 3, (5, d))).astype(np.float32)
        n_o = CLASSES[name][4]
        orth = None
        if n_o:
            r2 = (x.astype(np.float64) ** 2).sum(axis=1)
            c = rng.normal(0, 1, (n_o, d + 1))
            orth = np.stack([(c[j, 0] + x.astype(np.float64) @ c[j, 1:]) * np.exp(-0.5 * r2 / (1.0 + j)) for j in range(n_o)])
        _INPUTS[key] = (x, flat, x_bc, orth)
    return _INPUTS[key]


_ORACLE = {}


def oracle(name, N, traj=False):
    """fp64 oracle of (class, N), computed once per module run: one step (sums, gradient, fields, output jets, parameters after Adam)
    and, on request, the 9-step trajectory of its optimiser"""
    key = (name, N)
    kw = CLASSES[name][0]
    pb = go.Problem(**kw)
    x, flat, x_bc, orth = inputs(name, N)
    f64 = flat.astype(np.float64)
    if key not in _ORACLE:
        osc, ograd, ores = go.full_loss_and_grad(pb, f64, x.astype(np.float64), x_bc.astype(np.float64), orth=orth)
        _, oskip, oplain = go.expand_layers(pb.layers, pb.net_kind)
        ojets, _ = go.mlp_forward(go.unflatten(f64, pb.layers, pb.net_kind), x.astype(np.float64), pb.activation, skip=oskip, plain_tanh=oplain)
        new, _, _ = go.optimizer_step(go.OptState(lr0=1e-3), flat, ograd, osc["loss"])
        _ORACLE[key] = dict(sc=osc, grad=ograd, res=ores, jets=ojets, new=new)
    o = _ORACLE[key]
    if traj and "traj" not in o:
        _, tr = go.train_steps(pb, go.OptState(lr0=1e-3), f64, x.astype(np.float64), 9, x_bc.astype(np.float64), orth=orth, dtype=np.float64)
        o["traj"] = np.array([t["loss"] for t in tr])
    return o


@contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def make(name, N, x, flat, x_bc, orth):
    kw, _, path, _, _ = CLASSES[name]
    extra = {} if path is None else dict(path=path)
    eng = Engine(cfg_from_problem(go.Problem(**kw), **extra))
    eng.set_params(flat)
    eng.bind_points(torch.as_tensor(x, device="cuda"))
    eng.bind_boundary(torch.as_tensor(x_bc, device="cuda"))
    if orth is not None:
        for j in range(orth.shape[0]):
            eng.bind_orth(j, orth[j].astype(np.float32))
    return eng


def run_cell(name, N, env, multi=False, dp=False):
    """the engine of one cell, created, run and closed while `env` is set"""
    x, flat, x_bc, orth = inputs(name, N)
    with environment(env):
        eng = make(name, N, x, flat, x_bc, orth)
        try:
            out = dict(kern=eng.active_kernels, path=eng.active_path)
            out["jets"] = eng.forward_jets(torch.as_tensor(x, device="cuda")).cpu().numpy()
            rs, psi, res = eng.residual()
            out.update(rs=rs, psi=psi.cpu().numpy(), res=res.cpu().numpy())
            if dp:
                eng.comm_init(0, 1)
                eng.step_dp()
                out["sc"] = eng.read_scalars()
            else:
                out["sc"] = eng.step()
            out["grad"] = eng.get_grad()
            out["params"] = eng.get_params()
            if multi:
                eng.run(8)
                out["losses"] = np.array([h["loss"] for h in eng.read_history(1, 9)])
                out["params9"] = eng.get_params()
        finally:
            eng.close()
    return out


def check_oracle(cell, o, multi, name):
    """failures of one cell of class `name` against the fp64 oracle (tolerances of test_step_matches_oracle, and the gradient per
    parameter block)"""
    bad = []
    osc = o["sc"]
    for c in range(cell["jets"].shape[0]):
        if not close(cell["jets"][c], o["jets"][c], 1e-5, 2e-6):
            bad.append(f"jet channel {c}: err {np.abs(cell['jets'][c] - o['jets'][c]).max():.3e}")
    if not close(cell["psi"], o["res"]["psi"], 5e-6, 2e-6):
        bad.append("residual(): psi")
    if not close(cell["res"], o["res"]["residual"], 2e-5, 1e-5):
        bad.append("residual(): residual")
    if abs(cell["rs"]["loss"] - osc["loss"]) > 1e-4 * abs(osc["loss"]):
        bad.append(f"residual(): loss {cell['rs']['loss']:.9g} vs {osc['loss']:.9g}")
    sc = cell["sc"]
    for k, tol in (("mu", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("bc", 1e-4), ("norm", 2e-4), ("sym", 1e-4), ("riesz", 1e-4), ("reg", 1e-4),
                   ("orth", 1e-4)):
        if abs(sc[k] - osc[k]) > tol * max(abs(osc[k]), 1e-6):
            bad.append(f"{k} {sc[k]:.9g} vs oracle {osc[k]:.9g}")
    eg = Hl.rel_err(cell["grad"], o["grad"])
    if not eg < 5e-5:
        bad.append(f"gradient rel err {eg:.3e}")
    kw = CLASSES[name][0]
    bad += Hl.block_failures(cell["grad"], o["grad"], kw["layers"], kw.get("net_kind", go.NET_MLP))
    d = np.abs(cell["params"] - o["new"])
    if not (np.quantile(d, 0.99) < 2e-5 and d.max() < 2.1e-3):
        bad.append(f"parameters after Adam: q99 {np.quantile(d, 0.99):.3e} max {d.max():.3e}")
    if multi:
        tr = o["traj"]
        dev = max(abs(a - t) / max(abs(t), 1e-30) / (1 + k) for k, (a, t) in enumerate(zip(cell["losses"], tr)))
        if not dev < 1e-3:
            bad.append(f"9-step loss trajectory off the oracle's: {dev:.3e}")
    return bad


def check_bitwise(cell, ref, multi):
    bad = []
    for k in ("loss", "mu", "pde", "bc", "norm", "sym"):
        if cell["sc"][k] != ref["sc"][k]:
            bad.append(f"{k} {cell['sc'][k]!r} != default {ref['sc'][k]!r}")
    for k in ("grad", "params") + (("losses", "params9") if multi else ()):
        if not np.array_equal(cell[k], ref[k]):
            bad.append(f"{k} differs from the default engine's bits")
    return bad


_DEFAULT = {}


def default_cell(name, bi):
    """the class's engine under its batch's base environment only (with the 9-step run, for the bitwise rows)"""
    if (name, bi) not in _DEFAULT:
        N, base, _ = CLASSES[name][1][bi]
        _DEFAULT[(name, bi)] = run_cell(name, N, base, multi=True)
    return _DEFAULT[(name, bi)]


def kstr(k):
    return ";".join(f"{a}={b}" for a, b in k.items())


SEEN = {}
DRIVEN = sorted(n for n, r in T.SWITCHES.items() if not r["expect"].startswith("elsewhere:"))


@pytest.mark.parametrize("switch", DRIVEN)
def test_switch_against_the_oracle(switch):
    row = T.SWITCHES[switch]
    expect, multi, dp = row["expect"], row.get("multi", False), row.get("dp", False)
    fails, differs, cells = [], [], 0
    for name, bi in CELLS:
        if not row["applies_to"](descriptor(name, bi)):
            continue
        N, base, _ = CLASSES[name][1][bi]
        ref = default_cell(name, bi)
        for val in row["values"]:
            env = dict(base, **val)
            cells += 1
            try:
                cell = run_cell(name, N, env, multi=multi, dp=dp)
            except (ValueError, gpe_pinn.GPEError) as ex:
                fails.append(f"[{name} N={N} {env}] engine error: {ex}")
                continue
            tag = f"[{name} N={N} {env} -> {kstr(cell['kern'])}]"
            SEEN.setdefault(switch, []).append(dict(cls=name, N=N, env=env, kernels=kstr(cell["kern"]), default=kstr(ref["kern"])))
            if cell["kern"] != ref["kern"] or cell["path"] != ref["path"]:
                differs.append(tag)
            fails += [f"{tag} {m}" for m in check_oracle(cell, oracle(name, N, traj=multi), multi, name)]
            if expect == "bitwise":
                fails += [f"{tag} {m}" for m in check_bitwise(cell, ref, multi)]
    assert cells > 0, f"{switch}: applies to no class of the matrix"
    if expect == "kernels":
        assert differs, f"{switch}: no applicable class ran other kernels than by default -- dead or mis-specified row"
    assert not fails, f"{switch}: {len(fails)} failing cell checks\n" + "\n".join(fails[:40])


STAND_INS = [(name, bi) for name, bi in CELLS if CLASSES[name][1][bi][2] is not None]


@pytest.mark.parametrize("name,bi", STAND_INS, ids=[f"{n}-{CLASSES[n][1][b][0]}" for n, b in STAND_INS])
def test_large_batch_stand_ins_report_the_kernels_of_the_real_size(name, bi):
    """the threshold switches of a stand-in batch select, at a size the oracle can do, exactly what the default engine runs at the real
    size (binding the batch is enough to read the names: no step)"""
    N, base, real = CLASSES[name][1][bi]
    kw = CLASSES[name][0]
    d = kw["layers"][0]
    rng = np.random.default_rng(5)
    xr = rng.uniform(-3, 3, (real, d)).astype(np.float32)
    x, flat, x_bc, orth = inputs(name, N)
    big = make(name, real, xr, flat, x_bc, orth)
    kb = big.active_kernels
    big.close()
    torch.cuda.empty_cache()
    with environment(base):
        small = make(name, N, x, flat, x_bc, orth)
        ks = small.active_kernels
        small.close()
    assert ks == kb, f"{name}: stand-in N={N} {base} -> {kstr(ks)}; default at N={real} -> {kstr(kb)}"


@pytest.mark.parametrize("name", ["res1_1d_64", "res2_2d_32"])
def test_residual_networks_keep_the_cooperative_kernels_with_gpe_coop_0(name):
    """GPE_COOP=0 used to move residual-block networks onto f_forward / f_backward, which evaluate a plain MLP without the skip
    connection: loss, gradient and mu silently wrong.  The cooperative <..., RES> kernels are the only fused ones that know the blocks."""
    N, _, _ = CLASSES[name][1][0]
    cell = run_cell(name, N, {"GPE_COOP": "0"})
    k = cell["kern"]
    bad = check_oracle(cell, oracle(name, N), False, name)
    if not (cell["path"] == gpe_pinn.PATH_FUSED and k["fwd"].startswith("f_forward_coop<") and k["bwd"].startswith("f_backward_coop<")):
        bad.append("not the cooperative residual kernels")
    assert not bad, f"{name} GPE_COOP=0 {kstr(k)}: " + "; ".join(bad)


@pytest.mark.parametrize("name,b6", [("ns_2d_64x4_g500", True), ("1d_h32_2maps_hermite", True), ("2d_64_5maps", False),
                                     ("res1_1d_64", False), ("res2_2d_32", False)])
def test_b6_suffix_only_where_the_b6_reverse_kernel_runs(name, b6):
    """GPE_BWD_B6=1 takes f_backward_coop<..., B6> for plain MLPs of one to three maps only; residual blocks and four / five maps run the
    fp32 f_backward_coop, and their reverse kernel's name must not claim the bf16 form"""
    N, _, _ = CLASSES[name][1][0]
    x, flat, x_bc, orth = inputs(name, N)
    with environment({"GPE_BWD_B6": "1"}):
        eng = make(name, N, x, flat, x_bc, orth)
        k = eng.active_kernels
        eng.close()
    assert k["bwd"].startswith("f_backward_coop<") and k["bwd"].endswith(",b6>") == b6, k


@pytest.mark.parametrize("v", ["3", "4", "0"])
def test_forward_workgroups_per_cu_beyond_the_build_are_refused(v):
    """f_forward is compiled for GPE_FWD_WAVES (2) resident workgroups per CU: gpe_create refuses a count this build cannot honour"""
    x, flat, x_bc, orth = inputs("ns_2d_64x4_g500", 777)
    with environment({"GPE_FWD_WG_PER_CU": v}):
        with pytest.raises(ValueError, match="GPE_FWD_WG_PER_CU"):
            make("ns_2d_64x4_g500", 777, x, flat, x_bc, orth)


def test_kernel_names_seen_per_row():
    """(report) every kernels row changed what ran in at least one class; the names seen are written where SWITCH_MATRIX_REPORT points"""
    out = os.environ.get("SWITCH_MATRIX_REPORT")
    if out and SEEN:
        with open(out, "w") as f:
            json.dump(SEEN, f, indent=1)
    for switch, cells in SEEN.items():
        if T.SWITCHES[switch]["expect"] == "kernels":
            assert any(c["kernels"] != c["default"] for c in cells), switch
