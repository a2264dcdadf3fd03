#!/usr/bin/env python3
"""Launch BITS: for every kernel form the fused launchers can pick, three steps on N collocation + 5 boundary points, and one line per
cell: active_kernels, the loss of each step as a hex float, a sha256 over the parameter and gradient bytes.  Networks: H = 32 / 64 with
one to five maps (real psi; 1D, 2D, 3D) and one to three maps (complex psi, 2D), one and two residual blocks (H = 64, 1D), H = 128 with
one, three, five maps (2D), and [2, 512, 512, 1] on the generic set; each at N = 33 (three tiles, the last ragged) and N = 6 200 (past
fuse_head_max: the head in k_head_pde), by default and under GPE_COOP=0, GPE_PIPE=0 and GPE_BWD_B6=1 GPE_FWD_B6=1 where
tests/switch_table.py says the switch applies to the class.  Run it once per library build (GPE_HIP_LIB=...) and diff the outputs: a
change of the launch code that is a refactor reproduces every line of every cell that two runs of one build reproduce.
usage: tools/launch_bits.py > bits.txt"""
import hashlib, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpe_pinn
from bench import reference_init
from oracle import gpe_oracle as go
from tests.switch_table import SWITCHES

SETTINGS = [("default", {}, None), ("coop0", {"GPE_COOP": "0"}, "GPE_COOP"), ("pipe0", {"GPE_PIPE": "0"}, "GPE_PIPE"),
            ("b6", {"GPE_BWD_B6": "1", "GPE_FWD_B6": "1"}, "GPE_BWD_B6")]


def networks():
    """name -> (config keywords, class descriptor as tests/switch_table.py reads it)"""
    nets = {}
    for H in (32, 64):
        for maps in range(1, 6):
            for dim in (1, 2, 3):
                nets[f"h{H}_m{maps}_{dim}d"] = (dict(layers=[dim] + [H] * (maps + 1) + [1]), dict(H=H, maps=maps, res=False, n_out=1, dim=dim, path="fused"))
        for maps in range(1, 4):
            nets[f"h{H}_m{maps}_2d_complex"] = (dict(layers=[2] + [H] * (maps + 1) + [2], complex_psi=True, omega_rot=0.8),
                                                dict(H=H, maps=maps, res=False, n_out=2, dim=2, path="fused"))
    for blocks in (1, 2):
        nets[f"res{blocks}_h64_1d"] = (dict(layers=[1] + [64] * (blocks + 1) + [1], net_kind=go.NET_RESIDUAL),
                                       dict(H=64, maps=2 * blocks, res=True, n_out=1, dim=1, path="fused"))
    for maps in (1, 3, 5):
        nets[f"h128_m{maps}_2d"] = (dict(layers=[2] + [128] * (maps + 1) + [1]), dict(H=128, maps=maps, res=False, n_out=1, dim=2, path="wide"))
    nets["g512_2d"] = (dict(layers=[2, 512, 512, 1]), dict(H=512, maps=1, res=False, n_out=1, dim=2, path="generic"))
    return nets


def cell(name, kw, N, env):
    layers, d = kw["layers"], kw["layers"][0]
    rng = np.random.default_rng(N)
    x = ((rng.random((N, d)) * 2 - 1) * 4).astype(np.float32)
    xb = ((rng.random((5, d)) * 2 - 1) * 4).astype(np.float32)
    xb[:, 0] = np.float32(4.0)
    for k, v in env.items():
        os.environ[k] = v
    try:
        eng = gpe_pinn.Engine(gpe_pinn.GPEConfig(gamma=10.0, p=3, kinetic_coeff=0.5, pot_scale=0.5, dx=8.0 ** d / N, w_bc=10.0, w_norm=20.0,
                                                 lr=1e-3, **kw))
    finally:
        for k in env:
            del os.environ[k]
    eng.set_params(reference_init(layers, seed=1) if "net_kind" not in kw
                   else (np.random.default_rng(1).normal(0, 1, go.param_count(layers, kw["net_kind"])) * 0.2).astype(np.float32))
    eng.bind_points(torch.as_tensor(x, device="cuda")); eng.bind_boundary(torch.as_tensor(xb, device="cuda"))
    h, losses = hashlib.sha256(), []
    for _ in range(3):
        losses.append(float(eng.step()["loss"]).hex())
        h.update(np.asarray(eng.get_grad()).tobytes()); h.update(np.asarray(eng.get_params()).tobytes())
    k = eng.active_kernels
    eng.close()
    return f"{';'.join(f'{a}={b}' for a, b in k.items())} | {' '.join(losses)} | {h.hexdigest()[:16]}"


for name, (kw, desc) in networks().items():
    for N in (33, 6200):
        for tag, env, switch in SETTINGS:
            if switch and not SWITCHES[switch]["applies_to"](dict(desc, loss="plain", pad=False, large=False, P=0)):
                continue
            try:
                print(f"{name} N={N} {tag}: {cell(name, kw, N, env)}", flush=True)
            except Exception as ex:          # noqa: BLE001 -- reported per cell
                print(f"{name} N={N} {tag}: EXC {str(ex)[:200]}", flush=True)
