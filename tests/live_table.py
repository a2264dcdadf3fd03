"""Every way a caller changes a LIVE engine between two run() calls -- setters, rebinds, optimiser state, detours through the forward-only
entry points -- as one table.  gpe_run replays captured 8-step graphs; a capture bakes by-value arguments, pointers and host-side branch
outcomes into its nodes, and graph_key_of() (csrc/gpe_engine.hip) is the hand-kept list that decides when a capture is rebuilt.  A row
here is one change that list must notice (or that must not matter).  tests/test_gpu_live_engine.py runs every (row, class) cell on the
GPU; tests/test_live_table_cpu.py holds the table to include/gpe_hip.h (every gpe_set_* / gpe_bind_* entry point has a row or a written
exemption) and to the fp64 oracle (the old and the new problem of a row are far apart, so a stale replay cannot pass).

The state of a cell is a plain dict `ctx` (numpy only): what oracle(ctx) needs and what bind_all(eng, ctx) binds.
  cls, kw (oracle Problem keywords), N, path, x, V, flat, x_bc, tgt, q, W, orth {slot: array}, orth_state, base_pre, g (mixture
  couplings), sampler, monitor, keeper, engine_kw (GPEConfig overrides), env (switches set around engine creation)

Row fields
  group       the paragraph of the table the row belongs to
  classes     the network classes (CLASSES) the row makes sense for
  prep        ctx -> None: what the start state needs beyond the class (bound weights, an orth array, a precomputed potential ...)
  new         ctx -> ctx2, pure: the problem AFTER the mutation -- oracle(ctx2) is the fp64 answer the next step must give
  mutate      (eng, ctx2) -> None: the calls on the engine
  check       "record"  step 9's history record against oracle(ctx2) at the parameters the engine holds after the mutation
              "update"  the loss at step 9 cannot move: theta_9 - theta_8 against oracle/update_ref.py with the new optimiser state
              "detour"  nothing may change: the detoured engine equals an undetoured one bit for bit (twin: the twin makes the call too)
  covers      the C entry points of include/gpe_hip.h the row exercises
  env         switches for both engines of the cell (GPE_MERGE_BC, GPE_GRAPH_STEPS), beside GPE_GRAPH
  note        what a stale replay would get wrong
"""
import copy
import dataclasses

import numpy as np

from oracle import gpe_oracle as go
from tests import mixture_cases as mc
from tests import mixture_ref as mr
from tests import weighted_ref as wr

# ---- one small shape per kernel family: all far below 16 384 points, so gpe_run replays without forcing ---------------------------------
_MIX = "fused_2d_64x3_N49"
CLASSES = {
    "coop": dict(kw=dict(layers=[1, 32, 32, 32, 1], activation=1, kinetic_coeff=1.0, pot_scale=1.0, gamma=5.0, base_mode=0,
                         perturb_scale=0.05, w_bc=1.0, dx=12 / 776), N=777),                     # fused cooperative kernels, two boundary points
    "h128": dict(kw=dict(layers=[2, 128, 128, 1], gamma=10.0, dx=0.01), N=300),
    "wide": dict(kw=dict(layers=[3, 256, 256, 1], gamma=100.0, omega=(1.0, 1.4, 2.0), dx=0.01), N=300),
    "generic": dict(kw=dict(layers=[2, 48, 64, 32, 1], gamma=10.0, dx=0.01), N=300, path="generic"),
    "res": dict(kw=dict(layers=[1, 64, 64, 64, 1], net_kind=go.NET_RESIDUAL, activation=1, kinetic_coeff=1.0, potential=go.POT_GAUSSIAN,
                        pot_a=0.5, gamma=30.0, p=3, base_mode=1, perturb_scale=0.05, w_bc=1.0, dx=0.03), N=333),
    "cplx": dict(kw=dict(layers=[2, 64, 64, 64, 2], complex_psi=True, gamma=30.0, omega_rot=0.8, dx=0.02), N=200),
    "mix": dict(kw=dict(layers=mc.CASES[_MIX][0], activation=mc.CASES[_MIX][3]), N=mc.CASES[_MIX][1], mix=True),
}
ALL = tuple(CLASSES)
NONMIX = tuple(c for c in ALL if c != "mix")
REAL = ("coop", "h128", "wide", "generic", "res")


def _parity():
    from tests import test_gpu_parity as P          # (the recipe of its _inputs / _scale; imported late: it pulls in torch)
    return P


def points(cls, n, shift=0.0, seed=0):
    """collocation points of a class by the recipe of tests/test_gpu_parity._inputs, moved by `shift` along every axis"""
    c = CLASSES[cls]
    if c.get("mix"):
        x = mc.inputs(c["kw"]["layers"], n, seed=seed)[0]
    else:
        x = _parity()._inputs(c["kw"], n, seed=seed)[0]
    return (x + np.float32(shift)).astype(np.float32)


def start(cls, row=None):
    """the start state of a cell: the class's inputs, then the row's prep"""
    c = CLASSES[cls]
    kw = copy.deepcopy(c["kw"])
    N = c["N"]
    ctx = dict(cls=cls, kw=kw, N=N, path=c.get("path", "auto"), mix=bool(c.get("mix")), V=None, tgt=None, q=None, W=None, orth={},
               orth_state=None, base_pre=None, g=None, sampler=None, monitor=None, keeper=None, engine_kw={}, env={})
    if ctx["mix"]:
        ctx["x"], ctx["flat"], ctx["x_bc"], ctx["tgt"] = mc.inputs(kw["layers"], N, seed=4)
        ctx["g"] = tuple(mc.G)
    else:
        P = _parity()
        ctx["x"], ctx["flat"], ctx["x_bc"] = P._inputs(kw, N, scale=P._scale(kw))
    if row is not None:
        ctx["env"] = dict(row.get("env", {}))
        if row.get("prep"):
            row["prep"](ctx)
    return ctx


def problem(ctx):
    if ctx["mix"]:
        return mc.problem(ctx["kw"]["layers"], ctx["N"], ctx["kw"]["activation"], g=ctx["g"],
                          **{k: v for k, v in ctx["kw"].items() if k not in ("layers", "activation")})
    return go.Problem(**ctx["kw"])


def frozen_psi(ctx, st):
    """amplitude * (perturb_scale * NN_theta + phi_base_mode) on the bound points in fp64: what gpe_bind_orth_state evaluates"""
    pb = go.Problem(**{**ctx["kw"], "base_mode": st["base_mode"]})
    _, skip, plain = go.expand_layers(pb.layers, pb.net_kind)
    x64 = np.asarray(ctx["x"], np.float64)
    out, _ = go.mlp_forward(go.unflatten(np.asarray(st["theta"], np.float64), pb.layers, pb.net_kind), x64, pb.activation, value_only=True,
                            skip=skip, plain_tanh=plain)
    v = st["perturb_scale"] * out[0, :, 0]
    if st["base_mode"] >= 0:
        v = v + go.base_functions(pb, x64[:, 0])[0]
    return st["amplitude"] * v


def orth_rows(ctx):
    rows = dict(ctx["orth"])
    if ctx["orth_state"] is not None:
        rows[0] = frozen_psi(ctx, ctx["orth_state"])
    if not rows:
        return None
    assert sorted(rows) == list(range(len(rows)))
    return np.stack([np.asarray(rows[k], np.float64) for k in sorted(rows)])


def oracle(ctx, flat=None):
    """fp64 scalars (loss, mu, ...) of the step the engine must take from the state ctx describes, at the parameters `flat`"""
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    flat = f64(ctx["flat"] if flat is None else flat)
    pb = problem(ctx)
    if ctx["mix"]:
        sc = mr.loss_and_grad(pb, flat, f64(ctx["x"]), f64(ctx["x_bc"]), f64(ctx["tgt"]), q=f64(ctx["q"]), W=ctx["W"])[0]
        sc = dict(sc); sc["mu"] = sc["mu1"]
        return sc
    if ctx["q"] is not None:
        assert ctx["V"] is None and ctx["base_pre"] is None
        return wr.weighted_loss_and_grad(pb, flat, ctx["x"], ctx["q"], f64(ctx["x_bc"]), f64(ctx["tgt"]), orth_rows(ctx), ctx["W"])[0]
    return go.full_loss_and_grad(pb, flat, f64(ctx["x"]), f64(ctx["x_bc"]), f64(ctx["tgt"]), f64(ctx["V"]), orth_rows(ctx),
                                 base_pre=ctx["base_pre"])[0]


# ---- binding a state to an engine (GPU side; torch only through the engine's own conversions) --------------------------------------------
def config(ctx):
    if ctx["mix"]:
        from tests.test_gpu_mixture import config as mix_config
        return mix_config(problem(ctx), ctx["path"], **ctx["engine_kw"])
    P = _parity()
    return P.cfg_from_problem(problem(ctx), path=P.PATHS[ctx["path"]] if ctx["path"] != "auto" else 0, **ctx["engine_kw"])


def bind_all(eng, ctx):
    eng.set_params(ctx["flat"])
    if ctx["sampler"] is not None:
        bind_sampler(eng, ctx["sampler"])
    else:
        eng.bind_points(ctx["x"], V=ctx["V"])
    if ctx["x_bc"] is not None:
        eng.bind_boundary(ctx["x_bc"], ctx["tgt"])
    if ctx["base_pre"] is not None:
        eng.bind_base(*ctx["base_pre"])
    for k, a in ctx["orth"].items():
        eng.bind_orth(k, a)
    if ctx["orth_state"] is not None:
        bind_state(eng, ctx["orth_state"])
    if ctx["q"] is not None and (ctx["sampler"] is None or "edges" not in ctx["sampler"]):
        eng.bind_weights(ctx["q"], ctx["W"])
    if ctx["monitor"] is not None:
        eng.bind_monitor(ctx["monitor"]["x"], every=ctx["monitor"]["every"], dv=ctx["kw"]["dx"])
    if ctx["keeper"] is not None:
        eng.bind_keeper(**ctx["keeper"])


def bind_sampler(eng, s):
    if "edges" in s:
        eng.bind_sampler_graded(s["edges"], every=s["every"], seed=s["seed"])
    else:
        eng.bind_sampler(s["lo"], s["hi"], s["shape"], every=s["every"], seed=s["seed"])


def bind_state(eng, st, donor=False):
    if donor:                      # the frozen state taken from a second engine of the same network (closed again at once)
        cfg = dataclasses.replace(eng.cfg, base_mode=st["base_mode"], perturb_scale=st["perturb_scale"])
        other = type(eng)(cfg)
        try:
            other.set_params(st["theta"])
            eng.bind_orth_state(0, other, amplitude=st["amplitude"])
        finally:
            other.close()
    else:
        eng.bind_orth_state(0, st["theta"], base_mode=st["base_mode"], perturb_scale=st["perturb_scale"], amplitude=st["amplitude"])


# ---- building blocks of the rows --------------------------------------------------------------------------------------------------------
def _with(ctx, **ch):
    c2 = dict(ctx)
    c2["kw"] = dict(ctx["kw"]); c2["orth"] = dict(ctx["orth"])
    for k, v in ch.items():
        if k.startswith("kw_"):
            c2["kw"][k[3:]] = v
        else:
            c2[k] = v
    return c2


_W6 = ("w_pde", "w_bc", "w_norm", "w_sym", "w_orth", "w_riesz")
_W6_DEFAULT = dict(w_pde=1.0, w_bc=10.0, w_norm=20.0, w_sym=0.0, w_orth=0.0, w_riesz=0.0)


def _set_loss_weights(eng, c2):
    eng.set_loss_weights(*[float(c2["kw"].get(k, _W6_DEFAULT[k])) for k in _W6])


def _loss_weight_row(name, factor, classes, prep=None, note=""):
    def new(ctx):
        return _with(ctx, **{"kw_" + name: ctx["kw"].get(name, _W6_DEFAULT[name]) * factor})
    return dict(group="physics", classes=classes, prep=prep, new=new, mutate=_set_loss_weights, check="record",
                covers=("gpe_set_loss_weights",), note=note or f"{name} travels by value in Phys: the replay keeps the old weight")


def _gauss(ctx, centre, width=1.5):
    x = np.asarray(ctx["x"], np.float64)
    return np.exp(-((x - centre) ** 2).sum(axis=1) / (2 * width * width)).astype(np.float32)


def _prep_orth(slot_array=True, w=5.0):
    def prep(ctx):
        ctx["kw"]["w_orth"] = w
        if slot_array:
            ctx["orth"] = {0: _gauss(ctx, 0.5)}
    return prep


def _state_of(ctx, amplitude):
    P = _parity()
    kw = ctx["kw"]
    rng = np.random.default_rng(1001)
    theta = (rng.normal(0, 1, go.param_count(kw["layers"], kw.get("net_kind", 0))) * P._scale(kw)).astype(np.float32)
    return dict(theta=theta, base_mode=kw.get("base_mode", -1), perturb_scale=1.0 if kw.get("base_mode", -1) < 0 else 0.3, amplitude=amplitude)


def _prep_weights(ctx):
    ctx["q"] = np.random.default_rng(7).uniform(0.2, 3.0, ctx["N"]).astype(np.float32)


def _weighted(ctx):
    c2 = _with(ctx)
    _prep_weights(c2)
    return c2


def _prep_orth_tripled(ctx):
    _prep_orth(True)(ctx)
    ctx["orth"] = {0: 3.0 * ctx["orth"][0]}


def _prep_orth_state(ctx):
    _prep_orth(False)(ctx)
    ctx["orth_state"] = _state_of(ctx, 2.0)


def _new_points(dn, shift, with_V=False):
    def new(ctx):
        n = ctx["N"] + dn
        x = points(ctx["cls"], n, shift, seed=0 if dn == 0 else 3)
        V = None
        if with_V:
            V = (0.8 * (np.asarray(x, np.float64) ** 2).sum(axis=1) + 1.0).astype(np.float32)
        c2 = _with(ctx, x=x, N=n, V=V, q=None, W=None, sampler=None)
        if ctx["mix"]:                      # (mixture_cases.problem takes dx = 1 / N of the START: the engine's dx does not move with a bind)
            c2["kw"]["dx"] = problem(ctx).pb.dx
        return c2
    return new


def _bind_points(eng, c2):
    eng.bind_points(c2["x"], V=c2["V"])


def _refill_and_rebind(eng, c2):
    import torch
    t = eng._keep["x"]                      # the very tensor the engine reads: refilled in place, bound again (same pointer, same n)
    ptr = t.data_ptr()
    t.copy_(torch.as_tensor(c2["x"], device=t.device))
    eng.bind_points(t)
    assert eng._keep["x"].data_ptr() == ptr


def _prep_V(ctx):
    ctx["kw"]["potential"] = go.POT_PRECOMPUTED
    ctx["V"] = (0.5 * (np.asarray(ctx["x"], np.float64) ** 2).sum(axis=1)).astype(np.float32)


def _boundary(n_b, target_scale=1.5, seed=11):
    def new(ctx):
        d = ctx["kw"]["layers"][0]
        rng = np.random.default_rng(seed)
        xb = ctx["x_bc"] if n_b is None else rng.uniform(-3, 3, (n_b, d)).astype(np.float32)
        tgt = (rng.normal(0, 1, (xb.shape[0], ctx["kw"]["layers"][-1])) * target_scale).astype(np.float32)
        return _with(ctx, x_bc=xb, tgt=tgt)
    return new


def _bind_boundary(eng, c2):
    eng.bind_boundary(c2["x_bc"], c2["tgt"])


def merged(ctx):
    """the engine's rule (csrc/gpe_engine.hip: rebuild_main): the boundary rows ride in the collocation launch when 8 n_b <= N"""
    return ctx["env"].get("GPE_MERGE_BC", "1") != "0" and 8 * len(ctx["x_bc"]) <= ctx["N"]


def _sampler_spec(ctx, graded):
    d = ctx["kw"]["layers"][0]
    shape = [ctx["N"]] if d == 1 else ([15, ctx["N"] // 15] if d == 2 else [5, 6, ctx["N"] // 30])
    assert int(np.prod(shape)) == ctx["N"]
    if graded:
        from gpe_pinn import sampler as S
        return dict(edges=[S.sinh_edges(4.0, s, 1.5) + np.float32(1.0) for s in shape], every=1000, seed=5)
    return dict(lo=[-3.0] * d, hi=[5.0] * d, shape=shape, every=1000, seed=5)


def _sampled(ctx, s):
    from gpe_pinn import sampler as S
    if "edges" in s:
        return _with(ctx, x=S.graded_points(s["edges"], s["seed"], 0), q=S.graded_weights(s["edges"]), W=S.graded_total(s["edges"]), V=None,
                     sampler=s)
    return _with(ctx, x=S.stratified_points(s["lo"], s["hi"], s["shape"], s["seed"], 0), q=None, W=None, V=None, sampler=s)


def _prep_sampler(ctx):
    ctx.update(_sampled(ctx, _sampler_spec(ctx, graded=False)))


def _prep_keeper(ctx):
    """monitor every 4 steps, graphs of 4 steps (a replay must not run past a monitor step), min_delta = 1e30: the first record (step 4)
    improves on +inf, the second (step 8) cannot -- the keeper holds theta_4 whatever the metric does.  lr = 1e-2 moves theta_4 and
    theta_8 far enough apart for the fp64 oracle to tell them apart (tests/test_live_table_cpu.py follows the trajectory on the CPU)."""
    ctx["env"]["GPE_GRAPH_STEPS"] = "4"
    ctx["engine_kw"]["lr"] = 1e-2
    ctx["monitor"] = dict(x=np.linspace(-5, 5, 129, dtype=np.float32).reshape(-1, 1), every=4)
    ctx["keeper"] = dict(metric="res_rms", min_delta=1e30)


def _prep_base(ctx):
    ctx["kw"]["base_kind"] = go.BASE_PRECOMPUTED
    ctx["base_pre"] = tuple(a.astype(np.float32) for a in go.hermite_base(np.asarray(ctx["x"], np.float64)[:, 0], 0))


def _detour(call, covers=(), twin=False, classes=NONMIX, note=""):
    return dict(group="detours", classes=classes, prep=None, new=lambda ctx: ctx, mutate=call, check="detour", twin=twin, covers=covers, note=note)


def _d_forward(eng, c2):
    import torch
    d = c2["kw"]["layers"][0]
    other = torch.linspace(-2.0, 2.0, 100 * d, device="cuda").reshape(-1, d)
    assert torch.isfinite(eng.forward(other)).all()


def _d_mse(eng, c2):
    tgt = np.cos(np.asarray(c2["x"], np.float64).sum(axis=1, keepdims=True)) * np.ones((1, c2["kw"]["layers"][-1]))
    eng.bind_target(tgt.astype(np.float32))
    assert np.isfinite(eng.mse_step()["loss"])


ROWS = {
    # ---- physics setters: by-value members of Phys / OptCfg ------------------------------------------------------------------------------
    "set_gamma": dict(group="physics", classes=NONMIX, new=lambda c: _with(c, kw_gamma=c["kw"]["gamma"] * 8.0),
                      mutate=lambda e, c: e.set_gamma(c["kw"]["gamma"]), check="record", covers=("gpe_set_gamma",),
                      note="gamma is baked into head and seed nodes: the continuation would train on the old interaction strength"),
    "set_power": dict(group="physics", classes=("coop", "generic", "res"), new=lambda c: _with(c, kw_p=4),
                      mutate=lambda e, c: e.set_power(4), check="record", covers=("gpe_set_power",), note="p = 3 stays in the head (real psi)"),
    "set_perturb_scale": dict(group="physics", classes=("coop", "res"), new=lambda c: _with(c, kw_perturb_scale=0.6),
                              mutate=lambda e, c: e.set_perturb_scale(0.6), check="record", covers=("gpe_set_perturb_scale",),
                              note="u = phi_n + s NN with the old s: the perturbation loop of the reference never advances"),
    "set_n_global": dict(group="physics", classes=("coop", "h128", "cplx", "mix"), new=lambda c: _with(c, kw_n_global=8 * c["N"]),
                         mutate=lambda e, c: e.set_n_global(c["kw"]["n_global"]), check="record", covers=("gpe_set_n_global",),
                         note="N of the means (Phys.n_global, a double by value)"),
    "w_pde": _loss_weight_row("w_pde", 10.0, ("coop", "generic", "cplx", "mix")),
    "w_bc": _loss_weight_row("w_bc", 100.0, ("coop", "generic", "cplx", "mix"), prep=lambda c: c.update(_boundary(None)(c)),
                             note="w_bc scales the boundary seeds in the merged rows and in the side-stream batch alike"),
    "w_norm": _loss_weight_row("w_norm", 10.0, ("coop", "generic", "cplx", "mix")),
    "w_orth": _loss_weight_row("w_orth", 10.0, ("coop", "h128"), prep=_prep_orth(True, 2.0)),
    "w_riesz": _loss_weight_row("w_riesz", 10.0, ("coop", "wide"),
                                prep=lambda c: c["kw"].update(w_riesz=1.0, riesz_kind=go.RIESZ_VARIATIONAL)),
    "w_sym": _loss_weight_row("w_sym", 40.0, ("coop", "h128"), prep=lambda c: c["kw"].update(w_sym=5.0),
                              note="between two non-zero values: the symmetry batch exists on both sides, only the by-value weight moves"),
    "set_mixture": dict(group="physics", classes=("mix",), new=lambda c: _with(c, g=(2.0, 5.0, -1.5)),
                        mutate=lambda e, c: e.set_mixture(*c["g"]), check="record", covers=("gpe_set_mixture",),
                        note="the couplings live in OptCfg.mix and the head / seed nodes (as tests.test_gpu_mixture::"
                             "test_set_mixture_takes_effect_at_the_next_step, whose values these are)"),
    # ---- optimiser: device-resident state, nothing by value -- a capture must read it afresh ----------------------------------------------
    "set_lr": dict(group="optimiser", classes=("coop", "h128", "generic"), new=lambda c: _with(c, lr=3e-3),
                   mutate=lambda e, c: e.set_lr(c["lr"]), check="update", covers=("gpe_set_lr",), note="lr lives in OptDev on the device"),
    "reset_optimizer": dict(group="optimiser", classes=("coop", "h128", "generic"), new=lambda c: _with(c, lr=2e-3, adam="zero"),
                            mutate=lambda e, c: e.reset_optimizer(c["lr"]), check="update", covers=("gpe_reset_optimizer",),
                            note="moments zeroed, step 0: a replay that kept bias-correction powers by value would divide by the old ones"),
    "set_adam_state": dict(group="optimiser", classes=("coop", "h128", "generic"), new=lambda c: _with(c, adam="given"),
                           mutate=lambda e, c: e.set_adam_state(*adam_state(e.n_params)), check="update", covers=("gpe_set_adam_state",),
                           note="checkpoint restore: moments and step counter written from the host"),
    "set_params": dict(group="optimiser", classes=ALL,
                       new=lambda c: _with(c, flat=(c["flat"] * np.float32(-0.8) + np.float32(0.05)).astype(np.float32), params="set"),
                       mutate=lambda e, c: e.set_params(c["flat"]), check="record", covers=("gpe_set_params",),
                       note="packed weight copies must be rebuilt before the replayed forward pass reads them"),
    "keeper_restore": dict(group="optimiser", classes=("coop",), prep=_prep_keeper, new=lambda c: _with(c, params="kept"),
                           mutate=lambda e, c: e.restore_best(), check="record", covers=("gpe_keeper_restore",),
                           note="device-to-device copy of the kept parameters: packed copies stale unless the captured step repacks"),
    # ---- points ----------------------------------------------------------------------------------------------------------------------------
    "points_new_array": dict(group="points", classes=ALL, new=_new_points(0, 2.5), mutate=_bind_points, check="record", covers=("gpe_bind_points",),
                             note="same n, another pointer: Pts.a is a by-value kernel argument"),
    "points_refilled_in_place": dict(group="points", classes=("coop", "wide", "generic"), new=_new_points(0, -2.5), mutate=_refill_and_rebind,
                                     check="record", covers=("gpe_bind_points",),
                                     note="same pointer, same n: the key does not move and must not need to -- nothing derived from x may be cached"),
    "points_n_plus_1": dict(group="points", classes=("coop", "generic", "cplx"), new=_new_points(1, 1.5), mutate=_bind_points, check="record",
                            covers=("gpe_bind_points",), note="n, grids and (at a multiple of 64) ld change; batch buffers may be reallocated"),
    "points_n_minus_17": dict(group="points", classes=ALL, new=_new_points(-17, 1.5), mutate=_bind_points, check="record",
                              covers=("gpe_bind_points",),
                              note="fewer tiles, new activation buffers (S[], Z0 / Z1, A2, stored); the mixture's 32 points no longer carry its six "
                                   "boundary rows (8 n_b > N): merged -> batch of its own"),
    "points_with_V": dict(group="points", classes=("coop", "generic"), prep=_prep_V, new=_new_points(0, 1.5, with_V=True), mutate=_bind_points,
                          check="record", covers=("gpe_bind_points",), note="precomputed potential: Batch::V is a second caller pointer"),
    # ---- boundary --------------------------------------------------------------------------------------------------------------------------
    "boundary_new_target": dict(group="boundary", classes=("coop", "h128", "res", "mix"), new=_boundary(None), mutate=_bind_boundary,
                                check="record", covers=("gpe_bind_boundary",), note="bc_target: NULL -> array (another head branch), or another array"),
    "boundary_nb_5": dict(group="boundary", classes=("coop", "res"), new=_boundary(5), mutate=_bind_boundary, check="record",
                          covers=("gpe_bind_boundary",), note="n_b 2 -> 5: main.n (merged) or bc.n and the by-value boundary count of the update"),
    "boundary_flips_merge": dict(group="boundary", classes=("coop", "h128", "wide"), new=lambda c: _boundary(c["N"] // 8 + 1)(c),
                                 mutate=_bind_boundary, check="record", covers=("gpe_bind_boundary",),
                                 note="8 n_b > N: the rows leave the collocation launch for a batch of their own, forked to the side stream"),
    "boundary_flips_back": dict(group="boundary", classes=("coop", "h128"), prep=lambda c: c.update(_boundary(c["N"] // 8 + 1, seed=12)(c)),
                                new=_boundary(3), mutate=_bind_boundary, check="record", covers=("gpe_bind_boundary",),
                                note="own batch -> merged: the captured fork / join of the side stream must go"),
    "boundary_new_target_own_batch": dict(group="boundary", classes=("coop", "h128"), env={"GPE_MERGE_BC": "0"}, new=_boundary(None),
                                          mutate=_bind_boundary, check="record", covers=("gpe_bind_boundary",),
                                          note="GPE_MERGE_BC=0: the boundary batch is a side-stream fork INSIDE the capture"),
    "boundary_nb_own_batch": dict(group="boundary", classes=("coop", "h128", "res"), env={"GPE_MERGE_BC": "0"}, new=_boundary(7),
                                  mutate=_bind_boundary, check="record", covers=("gpe_bind_boundary",),
                                  note="GPE_MERGE_BC=0: bc.n and its buffers change inside the forked branch"),
    # ---- weights (<= 1 024 points: k_head_pde adds with one workgroup, the step is bit-reproducible) ---------------------------------------
    "weights_on": dict(group="weights", classes=("coop", "h128", "wide", "generic", "cplx", "mix"), new=_weighted,
                       mutate=lambda e, c: e.bind_weights(c["q"], c["W"]), check="record", covers=("gpe_bind_weights",),
                       note="the head leaves the forward kernel, the seeds the reverse kernel (weighted standalone kernels): a host-side branch"),
    "weights_off": dict(group="weights", classes=("coop", "generic", "mix"), prep=_prep_weights, new=lambda c: _with(c, q=None, W=None),
                        mutate=lambda e, c: e.bind_weights(None), check="record", covers=("gpe_bind_weights",),
                        note="back to the fused head / seed code and the count-based N"),
    "weights_total_only": dict(group="weights", classes=("coop", "h128", "mix"), prep=_prep_weights,
                               new=lambda c: _with(c, W=4.0 * float(np.asarray(c["q"], np.float64).sum())),
                               mutate=lambda e, c: e.bind_weights(e._keep["q"], c["W"]), check="record", covers=("gpe_bind_weights",),
                               note="same array, same pointer: only W (Phys.n_global) moves"),
    # ---- orthogonality / base --------------------------------------------------------------------------------------------------------------
    "orth_set": dict(group="orth", classes=("coop", "h128"), prep=_prep_orth(False), new=lambda c: _with(c, orth={0: 3.0 * _gauss(c, 0.5)}),
                     mutate=lambda e, c: e.bind_orth(0, c["orth"][0]), check="record", covers=("gpe_bind_orth",),
                     note="orth_host[] and Phys.n_orth 0 -> 1"),
    "orth_replaced": dict(group="orth", classes=("coop", "h128"), prep=_prep_orth(True), new=lambda c: _with(c, orth={0: -2.0 * _gauss(c, -1.0)}),
                          mutate=lambda e, c: e.bind_orth(0, c["orth"][0]), check="record", covers=("gpe_bind_orth",), note="another caller pointer"),
    "orth_cleared": dict(group="orth", classes=("coop", "h128"), prep=_prep_orth_tripled,
                         new=lambda c: _with(c, orth={}), mutate=lambda e, c: e.bind_orth(0, None), check="record", covers=("gpe_bind_orth",),
                         note="n_orth 1 -> 0: the overlap term must vanish from loss and seeds"),
    "orth_state_from_engine": dict(group="orth", classes=("coop", "h128"), prep=_prep_orth(False),
                                   new=lambda c: _with(c, orth_state=_state_of(c, 2.0)),
                                   mutate=lambda e, c: bind_state(e, c["orth_state"], donor=True), check="record", covers=("gpe_bind_orth_state",),
                                   note="frozen state taken from a second engine: an engine-owned buffer enters orth_host[]"),
    "orth_state_amplitude": dict(group="orth", classes=("coop", "h128"),
                                 prep=_prep_orth_state,
                                 new=lambda c: _with(c, orth_state=dict(c["orth_state"], amplitude=-5.0)),
                                 mutate=lambda e, c: bind_state(e, c["orth_state"]), check="record", covers=("gpe_bind_orth_state",),
                                 note="same slot, another amplitude: the buffer is refilled outside the graph, the replay must read the new values"),
    "bind_base": dict(group="orth", classes=("coop",), prep=_prep_base,
                      new=lambda c: _with(c, base_pre=tuple(a.astype(np.float32) for a in go.hermite_base(np.asarray(c["x"], np.float64)[:, 0], 2))),
                      mutate=lambda e, c: e.bind_base(*c["base_pre"]), check="record", covers=("gpe_bind_base",),
                      note="three more caller pointers (orth_host[4..6])"),
    # ---- sampler (every = 1000: no redraw inside the sixteen steps) -----------------------------------------------------------------------
    "sampler_bound": dict(group="sampler", classes=("coop", "h128", "wide"), new=lambda c: _sampled(c, _sampler_spec(c, False)),
                          mutate=lambda e, c: bind_sampler(e, c["sampler"]), check="record", covers=("gpe_bind_sampler",),
                          note="the engine's own point buffer replaces the caller's"),
    "sampler_graded_bound": dict(group="sampler", classes=("coop", "h128"), new=lambda c: _sampled(c, _sampler_spec(c, True)),
                                 mutate=lambda e, c: bind_sampler(e, c["sampler"]), check="record", covers=("gpe_bind_sampler_graded",),
                                 note="points AND weights become the engine's: pointer, wq, W and the weighted head / seed kernels at once"),
    "sampler_back_to_points": dict(group="sampler", classes=("coop", "h128"), prep=_prep_sampler, new=_new_points(0, -1.0), mutate=_bind_points,
                                   check="record", covers=("gpe_bind_points", "gpe_bind_sampler"),
                                   note="the sampler is cleared (its buffer freed) and the caller's points take over"),
    # ---- detours: nothing may change the next training step ----------------------------------------------------------------------------------
    "detour_residual": _detour(lambda e, c: e.residual(), classes=ALL,
                               note="forces k_begin, runs head and seeds standalone, leaves acc_clean / packed_dirty and the step record altered"),
    "detour_forward": _detour(_d_forward, note="another batch through the packed weights"),
    "detour_mse_step": _detour(_d_mse, covers=("gpe_bind_target",), twin=True, classes=("coop", "h128", "wide", "generic", "res", "cplx"),
                               note="moves the parameters through the value-only reverse kernels (the twin makes the same step): packed_dirty, "
                                    "the gradient buffer and Adam's moments are shared with the training step"),
    "detour_observables": _detour(lambda e, c: e.observables(), note="a temporary jet batch on the bound points, two reduction passes"),
}
for _r in ROWS.values():
    _r.setdefault("prep", None); _r.setdefault("env", {}); _r.setdefault("twin", False)

# entry points of the patterns tests/test_live_table_cpu.py looks for that have no row, each with its reason; "held by" names a test
EXEMPT = {
    "gpe_bind_monitor": "enqueues outside the graph (gpe_run cuts its replays at monitor steps) and writes nothing a step reads; held by "
                        "tests.test_gpu_observables::test_monitor_records_equal_stop_and_look; bound in the keeper_restore row",
    "gpe_bind_keeper": "two kernels behind a monitor record, never captured; held by tests.test_gpu_keeper::test_restore_best_and_step_on; "
                       "bound in the keeper_restore row",
    "gpe_use_external_exchange": "called once by Engine.__init__, before any capture exists; the two pointers it sets (grad, dbl) are in the key",
    "gpe_comm_set_async": "data-parallel entry points (gpe_step_dp / gpe_run_dp) never replay graphs",
}


def adam_state(P):
    rng = np.random.default_rng(9)
    return (rng.normal(0, 1e-2, P)).astype(np.float32), (rng.uniform(1e-6, 1e-3, P)).astype(np.float32), 5


def cells(check=None):
    return [(name, cls) for name, row in ROWS.items() for cls in row["classes"] if check is None or row["check"] == check]
