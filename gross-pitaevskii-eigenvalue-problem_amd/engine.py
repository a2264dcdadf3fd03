"""Host-side handle on the HIP engine (libgpe_hip.so).  PyTorch-ROCm tensors are used as device storage
and for torch.distributed (RCCL) only -- every number on the hot path is produced by the HIP kernels.

Replaces, for the hot path: the model/optimizer/scheduler objects and the epoch body of
refine/harmonic_pinn_simulation.py:295-361 and Gross_Pitaevskii_1D_power_Test.ipynb c10:L63-103.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch

from . import _capi as capi


class GPEError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[gpe status {code}] {msg}")
        self.code = code


@dataclass
class GPEConfig:
    """Python twin of include/gpe_hip.h:gpe_config (see the header for the reference citation of every field)."""
    layers: Sequence[int]
    activation: int = capi.ACT_TANH
    complex_psi: bool = False
    kinetic_coeff: float = 0.5
    potential: int = capi.POT_HARMONIC
    pot_scale: float = 0.5
    omega: Sequence[float] = (1.0, 1.0, 1.0)
    pot_a: float = 0.0
    pot_v0: float = 1.0
    pot_k: float = 2.0 * np.pi / 5.0
    omega_rot: float = 0.0
    gamma: float = 0.0
    p: int = 3
    abs_power: bool = False
    base_mode: int = -1
    base_deriv: int = 0
    perturb_scale: float = 1.0
    bc_nn_scale: float = 1.0
    w_pde: float = 1.0
    w_bc: float = 10.0
    w_norm: float = 20.0
    w_sym: float = 0.0
    w_orth: float = 0.0
    sym_sign: float = 1.0
    dx: float = 1.0
    n_global: int = 0
    lr: float = 1e-3
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    clip_norm: float = 1.0
    sched: int = capi.SCHED_CONST
    T_0: float = 200.0
    T_mult: float = 2.0
    eta_min: float = 1e-6
    factor: float = 0.5
    patience: int = 100
    min_lr: float = 1e-5
    threshold: float = 1e-4
    path: int = capi.PATH_AUTO
    world_size: int = 1
    history_capacity: int = 0
    stop_tol: float = 0.0
    stop_patience: int = 0
    base_kind: int = capi.BASE_HERMITE
    envelope: int = capi.ENV_NONE
    box_L: float = 1.0
    env_L: float = 1.0
    w_riesz: float = 0.0
    riesz_kind: int = capi.RIESZ_PAPER
    net_kind: int = capi.NET_MLP
    lambda_kind: int = capi.LAMBDA_RAYLEIGH      # LAMBDA_ENERGY: src/gross_pitaevskii_2D.py:192
    w_reg_f: float = 0.0                         # w / (mean u^2 + reg_f_eps)        src/gross_pitaevskii_2D.py:201
    reg_f_eps: float = 1e-2
    w_reg_lam: float = 0.0                       # w / (lambda^2 + reg_lam_eps)      src/gross_pitaevskii_2D.py:204
    reg_lam_eps: float = 1e-6
    mixture: bool = False                        # two real components u_1, u_2 on the two outputs (include/gpe_hip.h: gpe_config.mixture)
    mix_g: Sequence[float] = (0.0, 0.0, 0.0)     # (g11, g22, g12)
    mix_norm: Sequence[float] = (1.0, 1.0)       # target norms (n_1, n_2)

    def to_c(self) -> capi.gpe_config:
        c = capi.gpe_config()
        c.abi_version = capi.GPE_ABI_VERSION
        layers = [int(v) for v in self.layers]
        if len(layers) > capi.GPE_MAX_LAYERS:
            raise ValueError(f"at most {capi.GPE_MAX_LAYERS} layer entries")
        c.n_layers = len(layers)
        for i, v in enumerate(layers):
            c.layers[i] = v
        om = list(self.omega) + [1.0] * 3
        for i in range(3):
            c.omega[i] = float(om[i])
        for name in ("activation", "potential", "p", "base_mode", "base_deriv", "sched", "patience", "path",
                     "world_size", "history_capacity", "n_global", "stop_patience", "base_kind", "envelope", "riesz_kind", "net_kind", "lambda_kind"):
            setattr(c, name, int(getattr(self, name)))
        c.complex_psi = int(bool(self.complex_psi))
        c.abs_power = int(bool(self.abs_power))
        for name in ("kinetic_coeff", "pot_scale", "pot_a", "pot_v0", "pot_k", "omega_rot", "gamma", "perturb_scale",
                     "bc_nn_scale", "w_pde", "w_bc", "w_norm", "w_sym", "w_orth", "sym_sign", "dx", "lr", "beta1",
                     "beta2", "eps", "clip_norm", "T_0", "T_mult", "eta_min", "factor", "min_lr", "threshold",
                     "stop_tol", "box_L", "env_L", "w_riesz", "w_reg_f", "reg_f_eps", "w_reg_lam", "reg_lam_eps"):
            setattr(c, name, float(getattr(self, name)))
        c.mixture = int(bool(self.mixture))
        if len(self.mix_g) != 3 or len(self.mix_norm) != 2:
            raise ValueError("mix_g = (g11, g22, g12), mix_norm = (n1, n2)")
        for i in range(3):
            c.mix_g[i] = float(self.mix_g[i])
        for i in range(2):
            c.mix_norm[i] = float(self.mix_norm[i])
        return c

    @property
    def dim(self):
        return int(self.layers[0])

    @property
    def n_out(self):
        return int(self.layers[-1])

    @property
    def n_channels(self):
        return 1 + 2 * self.dim


class _DeviceArrayView:
    """A float32 device buffer the engine owns, described by the CUDA array interface so that torch can read it in place."""

    def __init__(self, ptr: int, shape, typestr: str = "<f4"):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)


def _check_dev_f32(t: torch.Tensor, name: str):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float32 tensor on the GPU")


def _store_get(store, key, timeout, rank):
    """ncclUniqueId from a key-value store, bounded in time: a rank whose key never appears (ranks that created a different number
    of communicators look up different default keys) must fail with the key's name instead of blocking for ever."""
    import time
    if hasattr(store, "wait"):                           # torch.distributed stores: a wait with its own timeout
        import datetime
        try:
            store.wait([key], datetime.timedelta(seconds=timeout))
        except Exception as ex:
            raise TimeoutError(f"comm_init: rank {rank} found no ncclUniqueId under store key {key!r} within {timeout:.0f} s "
                               f"(does every rank create its communicators in the same order / publish under this key?)") from ex
        return bytes(store.get(key))
    deadline = time.monotonic() + timeout
    while True:
        try:
            v = store.get(key)
        except KeyError:
            v = None
        if v is not None:
            return bytes(v)
        if time.monotonic() > deadline:
            raise TimeoutError(f"comm_init: rank {rank} found no ncclUniqueId under store key {key!r} within {timeout:.0f} s")
        time.sleep(0.01)


class Engine:
    """One engine per process per GPU.  The HIP extension is mandatory (no fallback)."""

    def __init__(self, cfg: GPEConfig, device: Optional[int] = None, use_torch_stream: bool = True):
        if not torch.cuda.is_available():
            raise GPEError(capi.GPE_ERR_HIP, "no GPU visible: the GPE engine has no CPU fallback")
        self.lib = capi.load()
        self.cfg = cfg
        self.device = torch.cuda.current_device() if device is None else int(device)
        torch.cuda.set_device(self.device)
        # kernels are enqueued on torch's current stream so that they are ordered with RCCL collectives
        stream = torch.cuda.current_stream(self.device).cuda_stream if use_torch_stream else 0
        self._h = C.c_void_p()
        ccfg = cfg.to_c()
        rc = self.lib.gpe_create(C.byref(ccfg), self.device, C.c_void_p(stream), C.byref(self._h))
        if rc != capi.GPE_OK:
            msg = self.lib.gpe_last_error(None)
            code = capi.GPE_ERR_INVALID if rc == capi.GPE_ERR_INVALID else rc
            err = msg.decode() if msg else "gpe_create failed"
            if rc == capi.GPE_ERR_INVALID:
                raise ValueError(err)          # the reference raises ValueError for bad problem descriptions
            raise GPEError(code, err)
        self.n_params = int(self.lib.gpe_param_count(self._h))
        self._keep = {}
        # caller-owned exchange buffers (so torch.distributed can all-reduce them in place)
        nd = int(self.lib.gpe_exchange_dbl_count())
        self._xdbl = torch.zeros(nd, dtype=torch.float64, device=f"cuda:{self.device}")
        gp, gn = C.c_void_p(), C.c_int64()                  # (length of the engine's gradient message: the network as it RUNS -- hidden
        self._chk(self.lib.gpe_exchange_grad(self._h, C.byref(gp), C.byref(gn)))     # widths without a kernel instance are zero-padded -- + 4)
        self._xgrad = torch.zeros(int(gn.value), dtype=torch.float32, device=f"cuda:{self.device}")
        self._chk(self.lib.gpe_use_external_exchange(self._h, C.c_void_p(self._xdbl.data_ptr()), nd,
                                                     C.c_void_p(self._xgrad.data_ptr()), self._xgrad.numel()))
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.lib.gpe_exchange_sums(self._h, C.byref(p), C.byref(n)))
        assert p.value == self._xdbl.data_ptr()
        self._sums_view = self._xdbl[: n.value]

    # ---- plumbing -----------------------------------------------------------------------------
    def _chk(self, rc):
        if rc != capi.GPE_OK:
            msg = self.lib.gpe_last_error(self._h)
            raise GPEError(rc, msg.decode() if msg else "?")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.gpe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def active_path(self) -> int:
        return int(self.lib.gpe_active_path(self._h))

    @property
    def active_kernels(self) -> dict:
        """{'fwd': name, 'bwd': name} of the jet forward / reverse kernels the bound collocation batch is dispatched to."""
        buf = C.create_string_buffer(512)
        self._chk(self.lib.gpe_active_kernels(self._h, buf, 512))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";"))

    # ---- data-parallel exchange inside the engine (RCCL on the engine's exchange stream) ---------------------------------
    _comm_seq = 0          # communicators created by this process: every rank creates them in the same order

    def comm_init(self, rank: int, world: int, store=None, key: str = None, timeout: float = 300.0):
        """Create the engine's own RCCL communicator.  The 128-byte ncclUniqueId of rank 0 reaches the other ranks through
        `store` (anything with set / get) or, when none is given, by torch.distributed.broadcast_object_list over the initialised
        default group.  `key`: the FULL store key, used as given (non-Python ranks can publish / read it under the same name); left
        at None it is "gpe_comm_id/<n>", n = communicators this process has created so far -- every rank must then create its
        communicators in the same order.  A rank that does not find the id within `timeout` seconds raises, naming the key."""
        if key is None:
            key = f"gpe_comm_id/{Engine._comm_seq}"
        Engine._comm_seq += 1
        ident = (C.c_ubyte * capi.GPE_COMM_ID_BYTES)()
        id_err = None
        if rank == 0:
            try:
                self._chk(self.lib.gpe_comm_unique_id(self._h, ident))
            except GPEError as ex:                         # (e.g. librccl not found) -- the other ranks are told below instead of left waiting
                if store is not None or world <= 1:
                    raise
                id_err = ex
        if store is not None:                              # caller's key-value store (set / get)
            if rank == 0:
                store.set(key, bytes(ident))
            else:
                C.memmove(ident, _store_get(store, key, timeout, rank), capi.GPE_COMM_ID_BYTES)
        elif world > 1:                                    # default: the initialised torch.distributed group, public API only
            import torch.distributed as dist
            box = [(bytes(ident) if id_err is None else None) if rank == 0 else None]
            dist.broadcast_object_list(box, src=0)
            if id_err is not None:
                raise id_err
            if box[0] is None:
                raise GPEError(capi.GPE_ERR_STATE, "comm_init: rank 0 could not create an ncclUniqueId")
            if rank != 0:
                C.memmove(ident, box[0], capi.GPE_COMM_ID_BYTES)
        self._chk(self.lib.gpe_comm_init(self._h, ident, int(rank), int(world)))

    def comm_info(self) -> dict:
        r, w, n = C.c_int(), C.c_int(), C.c_int64()
        self._chk(self.lib.gpe_comm_info(self._h, C.byref(r), C.byref(w), C.byref(n)))
        return dict(rank=r.value, world=w.value, collectives=n.value)

    def comm_destroy(self):
        self._chk(self.lib.gpe_comm_destroy(self._h))

    def comm_set_async(self, on: bool = True):
        """OPT-IN one-step-stale gradient (gradient all-reduce overlapped with the next forward); changes the trajectory."""
        self._chk(self.lib.gpe_comm_set_async(self._h, int(on)))

    def step_dp(self):
        """One data-parallel step with both exchanges issued by the engine (no Python between the phases, no host sync)."""
        self._chk(self.lib.gpe_step_dp(self._h))

    def run_dp(self, n_steps: int):
        self._chk(self.lib.gpe_run_dp(self._h, int(n_steps)))

    # ---- parameters ---------------------------------------------------------------------------------
    def set_params(self, flat):
        a = np.ascontiguousarray(np.asarray(flat, dtype=np.float32).ravel())
        self._chk(self.lib.gpe_set_params(self._h, a.ctypes.data_as(C.c_void_p), a.size))

    def get_params(self) -> np.ndarray:
        a = np.empty(self.n_params, dtype=np.float32)
        self._chk(self.lib.gpe_get_params(self._h, a.ctypes.data_as(C.c_void_p), a.size))
        return a

    def get_grad(self) -> np.ndarray:
        a = np.empty(self.n_params, dtype=np.float32)
        self._chk(self.lib.gpe_get_grad(self._h, a.ctypes.data_as(C.c_void_p), a.size))
        return a

    def get_adam_state(self):
        m = np.empty(self.n_params, dtype=np.float32)
        v = np.empty(self.n_params, dtype=np.float32)
        step = C.c_int64()
        self._chk(self.lib.gpe_get_adam_state(self._h, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p),
                                              m.size, C.byref(step)))
        return m, v, int(step.value)

    def set_adam_state(self, m, v, step):
        m = np.ascontiguousarray(m, dtype=np.float32)
        v = np.ascontiguousarray(v, dtype=np.float32)
        self._chk(self.lib.gpe_set_adam_state(self._h, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p),
                                              m.size, int(step)))

    def reset_optimizer(self, lr: float):
        self._chk(self.lib.gpe_reset_optimizer(self._h, float(lr)))

    # ---- data ---------------------------------------------------------------------------------------------
    def _to_dev(self, a, name):
        if isinstance(a, torch.Tensor):
            t = a.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        else:
            t = torch.as_tensor(np.asarray(a, dtype=np.float32), device=f"cuda:{self.device}").contiguous()
        _check_dev_f32(t, name)
        return t

    def bind_points(self, x, V=None):
        x = self._to_dev(x, "x")
        if x.dim() != 2 or x.shape[1] != self.cfg.dim:
            raise ValueError(f"x must be [N,{self.cfg.dim}]")
        Vt = None if V is None else self._to_dev(V, "V").reshape(-1)
        self._keep["x"], self._keep["V"] = x, Vt
        self._keep.pop("q", None)                            # (the engine drops bound weights at every bind of points)
        self._chk(self.lib.gpe_bind_points(self._h, C.c_void_p(x.data_ptr()), x.shape[0],
                                           C.c_void_p(Vt.data_ptr()) if Vt is not None else None))
        self.n_local = int(x.shape[0])

    def _sampler_spec(self, shape, edges, lo, hi, clip, seed, first, n, draw0, every):
        """(gpe_sampler_spec, [edge pointer or None] * 3) of the four sampler binds.  shape None: the grid is the edges' (shape[k] =
        len(edges[k]) - 1, lo / hi / default clip their end values); else lo / hi / shape describe it and edges, if any, must fit it.
        n None: the cells from `first` to the grid's last.  What the engine cannot honour it refuses itself (GPE_ERR_INVALID): nothing
        else is judged here.  (Each pointer keeps its numpy array alive.)"""
        from . import sampler
        per_axis_clip = lambda d: (sampler._per_axis(clip[0], d, "clip[0]"), sampler._per_axis(clip[1], d, "clip[1]"))
        if shape is None:                     # (the order of the checks is the order of the ValueErrors: edges, then clip ...)
            ed = sampler._edges(edges)
            d = len(ed)
            shp = [a.size - 1 for a in ed]
            lo32, hi32 = [a[0] for a in ed], [a[-1] for a in ed]
            clo, chi = (lo32, hi32) if clip is None else per_axis_clip(d)
        else:                                 # (... here shape, lo, hi, clip, then edges and their fit)
            shp = [int(v) for v in np.atleast_1d(np.asarray(shape)).ravel()]
            d = len(shp)
            if not 1 <= d <= capi.GPE_MAX_DIM:
                raise ValueError(f"shape: 1 to {capi.GPE_MAX_DIM} axes")
            lo32, hi32 = sampler._per_axis(lo, d, "lo"), sampler._per_axis(hi, d, "hi")
            clo, chi = (lo32, hi32) if clip is None else per_axis_clip(d)
            ed = None if edges is None else sampler._edges(edges)
            if ed is not None and [a.size - 1 for a in ed] != shp:
                raise ValueError("edges: shape[k] + 1 values per axis")
        sp = capi.gpe_sampler_spec()
        total = 1
        for k in range(d):
            sp.shape[k] = shp[k]
            sp.lo[k], sp.hi[k], sp.clip_lo[k], sp.clip_hi[k] = float(lo32[k]), float(hi32[k]), float(clo[k]), float(chi[k])
            total *= shp[k]
        sp.seed = int(seed) & (2 ** 64 - 1)
        sp.first_cell = int(first)
        sp.n_local = total - int(first) if n is None else int(n)
        sp.draw0, sp.every = int(draw0), int(every)
        return sp, [ed[k].ctypes.data_as(C.c_void_p) if ed is not None and k < d else None for k in range(3)]

    def bind_sampler(self, lo, hi, shape, every: int, seed: int = 0, first_cell: int = 0, n=None, draw0: int = 0, clip=None):
        """Device-side stratified sampler: the engine owns the collocation batch -- one uniformly placed point per cell of the grid of
        `shape` cells over [lo, hi], cells first_cell .. first_cell + n - 1 (n None: all of them) -- and redraws it in place every
        `every` steps on its own stream (no host synchronisation, a captured graph stays valid).  clip = (clip_lo, clip_hi) keeps the
        points inside a box narrower than the cells (default (lo, hi)).  sampler.stratified_points(lo, hi, shape, seed, draw, ...)
        rebuilds any set on the CPU, bit for bit."""
        sp, _ = self._sampler_spec(shape, None, lo, hi, clip, seed, first_cell, n, draw0, every)
        self._chk(self.lib.gpe_bind_sampler(self._h, C.byref(sp)))
        self._keep["x"], self._keep["V"] = None, None
        self.n_local = int(sp.n_local)

    def clear_sampler(self):
        """Drop the sampler and its buffer: no points stay bound."""
        self._chk(self.lib.gpe_bind_sampler(self._h, None))
        self.n_local = 0

    def sampler_points(self):
        """(copy of the set the sampler holds now as a [n, dim] device tensor, its draw index); synchronises."""
        p, n, d = C.c_void_p(), C.c_int64(), C.c_int64()
        self._chk(self.lib.gpe_sampler_points(self._h, C.byref(p), C.byref(n), C.byref(d)))
        view = _DeviceArrayView(p.value, (int(n.value), self.cfg.dim))      # the engine's buffer as a tensor, without owning it ...
        out = torch.as_tensor(view, device=f"cuda:{self.device}").clone()    # ... and the copy the caller keeps
        return out, int(d.value)

    # ---- analytic potential terms (include/gpe_hip.h: gpe_potential_terms; gpe_pinn/potential.py) -----------------------------------------
    def bind_potential_terms(self, terms):
        """Bind a table of analytic potential terms (potential.quadratic / quartic / gaussian / lattice / linear; at most
        potential.MAX_TERMS) on an engine configured with POT_PRECOMPUTED: the engine owns V from here on.  bind_points(x), the four
        samplers, observables(x) and bind_monitor(x, every) then work without V -- the engine fills its own array at every bind and
        behind every redraw.  On a live engine the sets the engine holds are refilled in stream order (no synchronisation; a captured
        graph stays valid).  Data-parallel: every rank binds the same table.  Checkpoints do not store it: bind it again after a load."""
        from . import potential
        terms = [terms] if isinstance(terms, potential.Term) else list(terms)
        arr = potential.to_c(terms)
        self._chk(self.lib.gpe_potential_terms(self._h, arr, len(terms)))

    def clear_potential_terms(self):
        """Drop the table.  Refused (GPE_ERR_STATE) while a sampler is bound or the monitor runs on an engine-evaluated V; points bound
        with the engine's V become unbound."""
        on_engine_v = self.lib.gpe_potential_values(self._h, None, None) == capi.GPE_OK      # the engine's own answer: the bound set runs on its V
        self._chk(self.lib.gpe_potential_terms(self._h, None, 0))
        if on_engine_v:
            self.n_local = 0
            self._keep["x"] = None

    def potential_terms(self) -> list:
        """The bound table as a list of potential.Term ([]: none bound)."""
        from . import potential
        arr, n = (capi.gpe_pot_term * capi.GPE_MAX_POT_TERMS)(), C.c_int32()
        self._chk(self.lib.gpe_potential_terms_read(self._h, arr, C.byref(n)))
        return potential.from_c(arr, int(n.value))

    def potential_values(self) -> torch.Tensor:
        """Copy of the engine-owned V [n_local] the bound collocation set runs on; synchronises."""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.lib.gpe_potential_values(self._h, C.byref(p), C.byref(n)))
        view = _DeviceArrayView(p.value, (int(n.value),))
        return torch.as_tensor(view, device=f"cuda:{self.device}").clone()

    def potential_at(self, x) -> torch.Tensor:
        """V of the bound terms on any points x [N, dim], by the kernel that fills the engine's own arrays; synchronises."""
        x = self._to_dev(x, "x")
        if x.dim() != 2 or x.shape[1] != self.cfg.dim:
            raise ValueError(f"x must be [N,{self.cfg.dim}]")
        out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
        self._chk(self.lib.gpe_potential_eval(self._h, C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(out.data_ptr())))
        return out

    # ---- per-point quadrature weights (include/gpe_hip.h: gpe_bind_weights) ---------------------------------------------------------------
    def bind_weights(self, q, total=None):
        """One weight q_i >= 0 per bound collocation row: every collocation sum takes q_i and every N of a mean becomes W = sum q over
        all ranks (total; None: this engine's own sum).  cfg.dx stays the multiplier it is -- with cell volumes as weights set dx = 1.
        bind_points / bind_sampler clear the weights; None clears them here."""
        if q is None:
            return self.clear_weights()
        t = self._to_dev(q, "q").reshape(-1)
        if t.numel() != getattr(self, "n_local", 0):
            raise ValueError(f"q must hold one weight per bound point ({getattr(self, 'n_local', 0)})")
        self._chk(self.lib.gpe_bind_weights(self._h, C.c_void_p(t.data_ptr()), 0.0 if total is None else float(total)))
        self._keep["q"] = t                                  # (kept only once the engine reads it: a refused bind leaves the old array bound)

    def clear_weights(self):
        self._chk(self.lib.gpe_bind_weights(self._h, None, 0.0))
        self._keep.pop("q", None)

    def weights(self) -> dict:
        """dict(q, local, total): a copy of the weights the step reads (the caller's, or the graded sampler's cell volumes) as a device
        tensor [n_local], this engine's sum of them and W; synchronises."""
        p, n, wl, wt = C.c_void_p(), C.c_int64(), C.c_double(), C.c_double()
        self._chk(self.lib.gpe_weights(self._h, C.byref(p), C.byref(n), C.byref(wl), C.byref(wt)))
        view = _DeviceArrayView(p.value, (int(n.value),))
        return dict(q=torch.as_tensor(view, device=f"cuda:{self.device}").clone(), local=wl.value, total=wt.value)

    def bind_sampler_graded(self, edges, every: int, seed: int = 0, first_cell: int = 0, n=None, draw0: int = 0, clip=None):
        """Graded stratified sampler: bind_sampler on the tensor-product grid whose cells are bounded by `edges` -- one strictly increasing
        array of cell edges per axis (shape[k] = len(edges[k]) - 1) -- with every point weighted by its cell's volume (bind_weights is
        implied; total = the whole grid's volume, so set cfg.dx = 1).  sampler.graded_points / graded_weights / graded_total rebuild
        points, weights and W on the CPU, bit for bit; sampler.sinh_edges makes centre-refined edges."""
        sp, ptrs = self._sampler_spec(None, edges, None, None, clip, seed, first_cell, n, draw0, every)
        self._chk(self.lib.gpe_bind_sampler_graded(self._h, C.byref(sp), *ptrs))
        self._keep["x"], self._keep["V"] = None, None
        self._keep.pop("q", None)
        self.n_local = int(sp.n_local)

    def bind_sampler_adaptive(self, edges, n_points: int, every: int, seed: int = 0, n_min: int = 1, uniform_share: float = 0.5,
                              clip=None, draw0: int = 0):
        """Residual-adaptive sampler: the cells bounded by `edges` (as for bind_sampler_graded) are blocks that share `n_points` rows
        among themselves anew at every redraw -- a share `uniform_share` in (0, 1] (kept as round(1024 * share) / 1024) by volume, the
        rest by the block's residual mass sum q r^2 of the state being trained, at least `n_min` rows each -- every row a uniformly
        placed point of its block with weight volume / rows (total = the grid's volume, so set cfg.dx = 1).  The bind allocates by
        volume.  sampler.adaptive_counts / adaptive_points / adaptive_weights rebuild counts, points and weights on the CPU, bit for
        bit, from adaptive_state().  Single-rank."""
        from . import sampler
        sp, ptrs = self._sampler_spec(None, edges, None, None, clip, seed, 0, None, draw0, every)
        self._chk(self.lib.gpe_sampler_adaptive(self._h, C.byref(sp), *ptrs, int(n_points), int(n_min),
                                                sampler.uniform_per_1024(uniform_share)))
        self._keep["x"], self._keep["V"] = None, None
        self._keep.pop("q", None)
        self.n_local = int(n_points)

    def bind_sampler_cells(self, cells, lo, hi, shape, every: int, seed: int = 0, clip=None, edges=None, first: int = 0, n_local=None,
                           draw0: int = 0):
        """Cell-subset sampler: bind_sampler (edges None) or bind_sampler_graded (edges: one array per axis, whose end values are lo / hi)
        on the cells of the strictly ascending int64 list `cells` alone -- a disk, a ball, any mask (sampler.ball_cells / mask_cells) --
        so the rows outside are never launched.  This engine holds rows first .. first + n_local - 1 of the list (n_local None: the rest).
        Uniform: set cfg.dx to the cell volume and n_global to len(cells); graded: the rows carry their cell volumes as weights with
        total = sampler.cells_total(cells, edges), so set cfg.dx = 1.  sampler.cells_points / cells_weights rebuild points and weights
        on the CPU, bit for bit."""
        c = np.ascontiguousarray(np.asarray(cells).ravel(), dtype=np.int64)
        if c.size == 0:
            raise ValueError("bind_sampler_cells: the list of cells is empty")
        sp, ptrs = self._sampler_spec(shape, edges, lo, hi, clip, seed, first, c.size - int(first) if n_local is None else n_local, draw0, every)
        self._chk(self.lib.gpe_sampler_cells(self._h, C.byref(sp), c.ctypes.data_as(C.c_void_p), c.size, *ptrs))
        self._keep["x"], self._keep["V"] = None, None
        self._keep.pop("q", None)
        self.n_local = int(sp.n_local)

    def sampler_cells(self):
        """(copy of the list of cells the engine holds as an int64 numpy array, this engine's first row in it); synchronises."""
        p, n, f = C.c_void_p(), C.c_int64(), C.c_int64()
        self._chk(self.lib.gpe_sampler_cells_read(self._h, C.byref(p), C.byref(n), C.byref(f)))
        view = _DeviceArrayView(p.value, (int(n.value),), "<i8")
        return torch.as_tensor(view, device=f"cuda:{self.device}").cpu().numpy().copy(), int(f.value)

    def adaptive_state(self) -> dict:
        """dict(mass, total, counts, draw): the block masses (float64 [B]) and their total that produced the counts (int32 [B]) of the
        set the adaptive sampler holds now -- zeros after the bind -- and that set's draw index; synchronises."""
        nb = C.c_int64()
        self._chk(self.lib.gpe_sampler_adaptive_blocks(self._h, C.byref(nb), None))       # the engine's own B sizes the host arrays
        B = int(nb.value)
        mass, counts = np.zeros(B, np.float64), np.zeros(B, np.int32)
        tot, d = C.c_double(), C.c_int64()
        self._chk(self.lib.gpe_sampler_adaptive_state(self._h, mass.ctypes.data_as(C.c_void_p), C.byref(tot),
                                                      counts.ctypes.data_as(C.c_void_p), C.byref(d)))
        return dict(mass=mass, total=tot.value, counts=counts, draw=int(d.value))

    def bind_boundary(self, xb, target=None):
        if xb is None:
            self._chk(self.lib.gpe_bind_boundary(self._h, None, 0, None))
            return
        xb = self._to_dev(xb, "xb")
        tg = None if target is None else self._to_dev(target, "target")
        self._keep["xb"], self._keep["tg"] = xb, tg
        self._chk(self.lib.gpe_bind_boundary(self._h, C.c_void_p(xb.data_ptr()), xb.shape[0],
                                             C.c_void_p(tg.data_ptr()) if tg is not None else None))

    def bind_base(self, phi, phi1, phi2):
        """GPE_BASE_PRECOMPUTED: base function and its first two derivatives on the bound points."""
        ts = [self._to_dev(a, "base").reshape(-1) for a in (phi, phi1, phi2)]
        self._keep["base"] = ts
        self._chk(self.lib.gpe_bind_base(self._h, *[C.c_void_p(t.data_ptr()) for t in ts]))

    def bind_orth(self, k: int, psi_k):
        t = None if psi_k is None else self._to_dev(psi_k, "psi_k").reshape(-1)
        self._keep[f"orth{k}"] = t
        self._chk(self.lib.gpe_bind_orth(self._h, int(k), C.c_void_p(t.data_ptr()) if t is not None else None))

    def bind_orth_state(self, k: int, params, base_mode: int = -1, perturb_scale: float = 1.0, amplitude: float = 1.0, which: str = "last"):
        """Frozen reference state in orthogonality slot k: psi_k = amplitude * (env * perturb_scale * NN_params + phi_base_mode), kept and
        evaluated by the engine on every collocation set it holds -- at the binds and behind every redraw of the sampler -- so that
        an excited state can be trained on sampler-drawn sets.  params: a flat parameter vector of this engine's network, or another
        Engine of the same network, whose get_params() and cfg.base_mode / cfg.perturb_scale are taken (the two keywords are then
        ignored); which = "best" takes that engine's kept parameters (best_params(), see bind_keeper) instead of its last.  None clears
        the slot."""
        if which not in ("last", "best"):
            raise ValueError('which: "last" or "best"')
        if which == "best" and not isinstance(params, Engine):
            raise ValueError('which="best" needs an Engine (with a keeper) as params')
        if params is None:
            self._chk(self.lib.gpe_bind_orth_state(self._h, int(k), None, 0, -1, 1.0, 1.0))
            self._keep.pop(f"orth{k}", None)
            return
        if isinstance(params, Engine):
            base_mode, perturb_scale = params.cfg.base_mode, params.cfg.perturb_scale
            params = params.best_params() if which == "best" else params.get_params()
        a = np.ascontiguousarray(np.asarray(params, dtype=np.float32).ravel())
        self._chk(self.lib.gpe_bind_orth_state(self._h, int(k), a.ctypes.data_as(C.c_void_p), a.size, int(base_mode),
                                               float(perturb_scale), float(amplitude)))
        self._keep.pop(f"orth{k}", None)            # the engine's own buffer replaced a caller array

    def orth_values(self, k: int) -> torch.Tensor:
        """Copy of the engine-owned psi_k [n_local] of the frozen state in slot k on the set bound now; synchronises."""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.lib.gpe_orth_values(self._h, int(k), C.byref(p), C.byref(n)))
        view = _DeviceArrayView(p.value, (int(n.value),))
        return torch.as_tensor(view, device=f"cuda:{self.device}").clone()

    # ---- forward-only -----------------------------------------------------------------------------------------
    def forward(self, x) -> torch.Tensor:
        x = self._to_dev(x, "x")
        out = torch.empty((x.shape[0], self.cfg.n_out), dtype=torch.float32, device=x.device)
        self._chk(self.lib.gpe_forward(self._h, C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(out.data_ptr())))
        return out

    def forward_jets(self, x) -> torch.Tensor:
        x = self._to_dev(x, "x")
        out = torch.empty((self.cfg.n_channels, x.shape[0], self.cfg.n_out), dtype=torch.float32, device=x.device)
        self._chk(self.lib.gpe_forward_jets(self._h, C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(out.data_ptr())))
        return out

    def residual(self, want_fields: bool = True):
        sc = capi.gpe_scalars()
        psi = res = None
        if want_fields:
            psi = torch.empty((self.n_local, self.cfg.n_out), dtype=torch.float32, device=f"cuda:{self.device}")
            res = torch.empty_like(psi)
        self._chk(self.lib.gpe_residual(self._h, C.byref(sc), C.c_void_p(psi.data_ptr()) if want_fields else None,
                                        C.c_void_p(res.data_ptr()) if want_fields else None))
        return sc.as_dict(), psi, res

    def eval_density(self, x, dx: float, abs_flag: bool = False):
        x = self._to_dev(x, "x")
        u = torch.empty((x.shape[0], self.cfg.n_out), dtype=torch.float32, device=x.device)
        dens = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
        self._chk(self.lib.gpe_eval_density(self._h, C.c_void_p(x.data_ptr()), x.shape[0], float(dx), int(abs_flag),
                                            C.c_void_p(u.data_ptr()), C.c_void_p(dens.data_ptr())))
        return u, dens

    # ---- training ---------------------------------------------------------------------------------------------------
    def step(self) -> dict:
        sc = capi.gpe_scalars()
        self._chk(self.lib.gpe_step(self._h, C.byref(sc)))
        return sc.as_dict()

    def run(self, n_steps: int):
        """n_steps steps enqueued back to back; no host synchronisation."""
        self._chk(self.lib.gpe_run(self._h, int(n_steps)))

    def step_begin(self):
        self._chk(self.lib.gpe_step_begin(self._h))

    def step_backward(self):
        self._chk(self.lib.gpe_step_backward(self._h))

    def step_update(self):
        self._chk(self.lib.gpe_step_update(self._h))

    @property
    def exchange_sums(self) -> torch.Tensor:
        """float64 device tensor (view) to all-reduce(sum) between step_begin and step_backward."""
        return self._sums_view

    @property
    def exchange_grad(self) -> torch.Tensor:
        """float32 device tensor [P+4] to all-reduce(sum) between step_backward and step_update."""
        return self._xgrad

    def step_distributed(self, group=None, sync: bool = False):
        """One data-parallel step: every rank holds a shard of the collocation points (dp.py)."""
        from .dp import distributed_step
        distributed_step(self, group)
        if sync:
            return self.read_scalars()
        return None

    def synchronize(self):
        self._chk(self.lib.gpe_synchronize(self._h))

    def stop_state(self):
        """(stopped, stop_step): early stopping evaluated on the device (refine/harmonic_pinn_simulation.py:389-400)."""
        s, st = C.c_int(), C.c_int64()
        self._chk(self.lib.gpe_stop_state(self._h, C.byref(s), C.byref(st)))
        return bool(s.value), int(st.value)

    def read_scalars(self) -> dict:
        sc = capi.gpe_scalars()
        self._chk(self.lib.gpe_read_scalars(self._h, C.byref(sc)))
        return sc.as_dict()

    def read_history(self, first_step: int, count: int):
        arr = (capi.gpe_scalars * count)()
        self._chk(self.lib.gpe_read_history(self._h, int(first_step), int(count), arr))
        return [a.as_dict() for a in arr]

    HISTORY_FIELDS = tuple(n for n, _ in capi.gpe_scalars._fields_)

    def read_history_array(self, first_step: int, count: int) -> np.ndarray:
        """The same records as one float64 array [count, len(HISTORY_FIELDS)] (no per-record Python objects: a 201-stage continuation
        reads 400 000 of them)."""
        arr = (capi.gpe_scalars * count)()
        self._chk(self.lib.gpe_read_history(self._h, int(first_step), int(count), arr))
        return np.frombuffer(arr, dtype=np.float64).reshape(count, len(self.HISTORY_FIELDS)).copy()

    # ---- observables of the current state, formed on the device (include/gpe_hip.h: struct gpe_observables) ------------------------------
    OBSERVABLE_FIELDS = ("n", "dv", "step", "norm", "kin", "pot", "inter", "rot", "energy", "mu", "mu_lap", "lz",
                         "mean_x0", "mean_x1", "mean_x2", "var_x0", "var_x1", "var_x2", "peak_density", "res_rms")

    def _obs_args(self, x, V, dv, name):
        x = self._to_dev(x, "x")
        if x.dim() != 2 or x.shape[1] != self.cfg.dim:
            raise ValueError(f"x must be [N,{self.cfg.dim}]")
        Vt = None if V is None else self._to_dev(V, "V").reshape(-1)
        if Vt is not None and Vt.numel() != x.shape[0]:
            raise ValueError("V must hold one value per point")
        self._keep[name + "_x"], self._keep[name + "_V"] = x, Vt
        return x, Vt, float(self.cfg.dx if dv is None else dv)

    # the entry points and the record of each kind of engine (scalar, mixture); the public methods below are thin pairs over these
    _OBS_KINDS = {False: dict(observables="gpe_observables", bind_monitor="gpe_bind_monitor", read_monitor="gpe_read_monitor",
                              bind_keeper="gpe_bind_keeper", record=capi.gpe_observables),
                  True: dict(observables="gpe_mixture_observables", bind_monitor="gpe_mixture_monitor", read_monitor="gpe_mixture_monitor_read",
                             bind_keeper="gpe_mixture_keeper", record=capi.gpe_mixture_observables)}

    def _obs_entry(self, mixture, name):
        return getattr(self.lib, self._OBS_KINDS[bool(mixture)][name])

    def _observables(self, mixture, x, V, dv) -> dict:
        fn, out = self._obs_entry(mixture, "observables"), self._OBS_KINDS[mixture]["record"]()
        if x is None:
            self._chk(fn(self._h, None, 0, None, float(self.cfg.dx if dv is None else dv), C.byref(out)))
        else:
            x, Vt, dv = self._obs_args(x, V, dv, "obs")
            self._chk(fn(self._h, C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(Vt.data_ptr()) if Vt is not None else None, dv, C.byref(out)))
        return out.as_dict()

    def _bind_monitor(self, mixture, x, every, V, dv, capacity):
        if x is None or every <= 0:
            return self.clear_monitor()
        x, Vt, dv = self._obs_args(x, V, dv, "mon")
        self._chk(self._obs_entry(mixture, "bind_monitor")(self._h, C.c_void_p(x.data_ptr()), x.shape[0],
                                                           C.c_void_p(Vt.data_ptr()) if Vt is not None else None, dv, int(every), int(capacity)))
        self._mon_cap = int(capacity) if capacity > 0 else 4096

    def _read_monitor_raw(self, first, count, mixture=False):
        avail = self.monitor_available()
        if count is None:                                   # everything from `first` on that the ring still holds
            first = max(int(first), avail - getattr(self, "_mon_cap", 4096), 0)
            count = max(avail - first, 0)
        arr = (self._OBS_KINDS[mixture]["record"] * max(int(count), 1))()
        if count > 0:
            self._chk(self._obs_entry(mixture, "read_monitor")(self._h, int(first), int(count), arr, None))
        return arr, int(count)

    def _read_monitor(self, mixture, first, count):
        arr, count = self._read_monitor_raw(first, count, mixture)
        return [arr[i].as_dict() for i in range(count)]

    def _read_monitor_array(self, mixture, first, count) -> np.ndarray:
        arr, count = self._read_monitor_raw(first, count, mixture)
        width = len(self.MIXTURE_OBSERVABLE_FIELDS if mixture else self.OBSERVABLE_FIELDS)
        return np.frombuffer(arr, dtype=np.float64).reshape(-1, width)[:count].copy()

    def _bind_keeper(self, mixture, metric, min_delta, patience):
        if metric not in self.KEEP_METRICS:
            raise ValueError(f"metric: one of {sorted(self.KEEP_METRICS)}")
        self._chk(self._obs_entry(mixture, "bind_keeper")(self._h, self.KEEP_METRICS[metric], float(min_delta), int(patience)))

    def observables(self, x=None, V=None, dv=None) -> dict:
        """E, mu, <L_z>, norm, moments, peak density and residual of the normalised state on the points x (None: the bound collocation
        points with their bound potential); dv: quadrature weight (None: cfg.dx).  What tools/accuracy_cfg4.py:state_numbers used to
        form on the host from forward_jets."""
        return self._observables(False, x, V, dv)

    def bind_monitor(self, x, every: int, V=None, dv=None, capacity: int = 0):
        """Held-out monitor: after every `every`-th step enqueued by step() / run() the observables on x are appended to a device ring
        (capacity 0: 4096 records) with no host synchronisation; read them with read_monitor()."""
        return self._bind_monitor(False, x, every, V, dv, capacity)

    def clear_monitor(self):
        self._chk(self.lib.gpe_bind_monitor(self._h, None, 0, None, 0.0, 0, 0))
        self._keep.pop("mon_x", None); self._keep.pop("mon_V", None)

    def monitor_available(self) -> int:
        """Records appended since bind_monitor / bind_mixture_monitor (synchronises); the ring keeps the newest `capacity` of them."""
        n = C.c_int64()
        self._chk(self._obs_entry(self.cfg.mixture, "read_monitor")(self._h, 0, 0, None, C.byref(n)))
        return int(n.value)

    def read_monitor(self, first: int = 0, count=None):
        """Monitor records [first, first+count) (0-based since bind_monitor; count None: up to the newest) as dicts."""
        return self._read_monitor(False, first, count)

    def read_monitor_array(self, first: int = 0, count=None) -> np.ndarray:
        """The same records as one float64 array [count, len(OBSERVABLE_FIELDS)]."""
        return self._read_monitor_array(False, first, count)

    # ---- keeper: the best parameters by the held-out monitor, kept on the device (include/gpe_hip.h: gpe_bind_keeper) -------------------
    KEEP_METRICS = {"res_rms": capi.KEEP_RES_RMS, "energy": capi.KEEP_ENERGY}

    # ---- mixture engines: observables, held-out monitor (include/gpe_hip.h: struct gpe_mixture_observables) -------------------------------
    MIXTURE_OBSERVABLE_FIELDS = ("n", "dv", "step", "norm1", "norm2", "kin1", "kin2", "pot1", "pot2", "inter11", "inter22", "inter12", "energy",
                                 "mu1", "mu2", "mu_lap1", "mu_lap2", "overlap") + \
        tuple(f"{k}{a}_{j}" for k in ("mean_x", "var_x") for a in (1, 2) for j in range(3)) + \
        ("peak_density1", "peak_density2", "res_rms1", "res_rms2", "res_rms_total")

    def mixture_observables(self, x=None, V=None, dv=None) -> dict:
        """Norms, energy parts, mu_a, overlap, moments, peak densities and residuals of the two-component state normalised to the target
        norms, on the points x (None: the bound collocation points with their bound potential and weights); dv: quadrature weight
        (None: cfg.dx).  Two-entry lists per component, inter = [11, 22, 12], mean_x / var_x [component][axis].  What
        tools/accuracy_mixture.py:state used to form on the host."""
        return self._observables(True, x, V, dv)

    def bind_mixture_monitor(self, x, every: int, V=None, dv=None, capacity: int = 0):
        """bind_monitor for a mixture engine: after every `every`-th step enqueued by step() / run() the mixture observables on x are
        appended to a device ring (capacity 0: 4096 records) with no host synchronisation; read them with read_mixture_monitor()."""
        return self._bind_monitor(True, x, every, V, dv, capacity)

    def read_mixture_monitor(self, first: int = 0, count=None):
        """Mixture monitor records [first, first+count) (0-based since bind_mixture_monitor; count None: up to the newest) as dicts."""
        return self._read_monitor(True, first, count)

    def read_mixture_monitor_array(self, first: int = 0, count=None) -> np.ndarray:
        """The same records as one float64 array [count, len(MIXTURE_OBSERVABLE_FIELDS)]."""
        return self._read_monitor_array(True, first, count)

    def bind_mixture_keeper(self, metric: str = "res_rms", min_delta: float = 0.0, patience: int = 0):
        """bind_keeper for a mixture engine: judges the mixture monitor's records by "res_rms" (res_rms_total) or "energy".  Needs
        bind_mixture_monitor first; keeper_state(), best_params(), best_record() (the mixture record) and restore_best() serve it."""
        self._bind_keeper(True, metric, min_delta, patience)

    def _keeper_read(self, *args):
        return (self.lib.gpe_mixture_keeper_read if self.cfg.mixture else self.lib.gpe_keeper_read)(self._h, *args)

    def bind_keeper(self, metric: str = "res_rms", min_delta: float = 0.0, patience: int = 0):
        """After every monitor record the engine compares `metric` ("res_rms" or "energy", lower is better) with the best so far and, on
        an improvement by more than min_delta, sets the parameters and the record aside -- on the device, with no host synchronisation.
        patience > 0: training stops (as by stop_tol / stop_patience) after that many records in a row without improvement.  Needs
        bind_monitor first; keeper.select restates the rule."""
        self._bind_keeper(False, metric, min_delta, patience)

    def clear_keeper(self):
        self._chk(self.lib.gpe_bind_keeper(self._h, capi.KEEP_NONE, 0.0, 0))

    def keeper_state(self) -> dict:
        """dict(seen, kept, since_best, stopped): records judged, records kept, records since the last one kept, and whether the keeper's
        patience stopped the optimiser; synchronises."""
        seen, kept, since, stopped = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        self._chk(self._keeper_read(None, 0, None, C.byref(seen), C.byref(kept), C.byref(since), C.byref(stopped)))
        return dict(seen=int(seen.value), kept=int(kept.value), since_best=int(since.value), stopped=bool(stopped.value))

    def best_params(self) -> np.ndarray:
        """The kept parameters (layout of get_params); GPEError while nothing is kept."""
        a = np.empty(self.n_params, dtype=np.float32)
        self._chk(self._keeper_read(a.ctypes.data_as(C.c_void_p), a.size, None, None, None, None, None))
        return a

    def best_record(self) -> dict:
        """The monitor record of the kept parameters, as read_monitor (a mixture engine: read_mixture_monitor) gives records."""
        out = capi.gpe_mixture_observables() if self.cfg.mixture else capi.gpe_observables()
        self._chk(self._keeper_read(None, 0, C.byref(out), None, None, None, None))
        return out.as_dict()

    def restore_best(self):
        """The kept parameters become the engine's parameters; Adam moments, scheduler state and the stop flag stay."""
        self._chk(self.lib.gpe_keeper_restore(self._h))

    # ---- pre-training on an analytic target (refine/harmonic_pinn_simulation.py:650-701) -----------------------------------
    def bind_target(self, target):
        t = None if target is None else self._to_dev(target, "target").reshape(-1, self.cfg.n_out)
        self._keep["target"] = t
        self._chk(self.lib.gpe_bind_target(self._h, C.c_void_p(t.data_ptr()) if t is not None else None))

    def mse_step(self) -> dict:
        sc = capi.gpe_scalars()
        self._chk(self.lib.gpe_mse_step(self._h, C.byref(sc)))
        return sc.as_dict()

    def mse_loss_grad(self):
        loss = C.c_double()
        self._chk(self.lib.gpe_mse_loss_grad(self._h, C.byref(loss)))
        return loss.value, self.get_grad()

    # ---- device-resident L-BFGS (torch.optim.LBFGS without a line search, flattened: include/gpe_hip.h) -----------------------
    LBFGS_FIELDS = ("loss", "grad_max", "grad_l1", "t", "gtd", "n_iter", "count", "frozen", "skipped", "pushed", "ys", "H_diag", "head",
                    "prev_loss")

    LBFGS_LS_FIELDS = ("phase", "ls_iter", "ls_evals", "evals_total", "t", "t_prev", "b0", "b1", "bf0", "bf1", "bgtd0", "bgtd1", "low_pos",
                       "f0", "gtd0", "dnorm", "accepted", "end_max_ls", "end_width", "end_curv", "stalled", "insuf_progress", "bslots",
                       "slot_new")
    LBFGS_LS_PHASES = ("none", "bracket", "zoom", "accepted", "frozen")
    LBFGS_FROZEN = ("live", "tolerance_grad", "nonfinite", "stop_loss", "keeper")      # lbfgs_read()["frozen"] indexes this

    def lbfgs_config(self, lr: float, history: int = 100, tolerance_grad: float = 1e-7, tolerance_change: float = 1e-9,
                     stop_loss: float = 0.0, line_search=None, c1: float = 1e-4, c2: float = 0.9, max_ls: int = 25):
        """Configure (torch's defaults) and reset the L-BFGS state.  The state freezes for good at max|g| <= tolerance_grad, on a
        non-finite loss or gradient, or at loss < stop_loss.  line_search: None (a fixed step lr) or "strong_wolfe" (torch's line search
        on the device; lbfgs_update() is then one TICK and lbfgs_run(n) spends n EVALUATIONS)."""
        if line_search not in (None, "strong_wolfe"):
            raise ValueError(f"line_search must be None or 'strong_wolfe', got {line_search!r}")
        self._chk(self.lib.gpe_lbfgs_config(self._h, float(lr), int(history), float(tolerance_grad), float(tolerance_change),
                                            float(stop_loss)))
        self._lbfgs_history = int(history)
        if line_search is not None or getattr(self, "_lbfgs_ls", False):      # (never made for an engine that never asked for one)
            self._chk(self.lib.gpe_lbfgs_line_search(self._h, 0 if line_search is None else 1, float(c1), float(c2), int(max_ls)))
            self._lbfgs_ls = line_search is not None

    def lbfgs_ls_read(self) -> dict:
        """The line search's record after the last tick (LBFGS_LS_FIELDS; phase as one of LBFGS_LS_PHASES); synchronises."""
        out = (C.c_double * len(self.LBFGS_LS_FIELDS))()
        self._chk(self.lib.gpe_lbfgs_ls_read(self._h, out))
        r = dict(zip(self.LBFGS_LS_FIELDS, out))
        for k in ("ls_iter", "ls_evals", "evals_total", "low_pos", "accepted", "end_max_ls", "end_width", "end_curv", "stalled",
                  "insuf_progress", "bslots", "slot_new"):
            r[k] = int(r[k])
        r["phase"] = self.LBFGS_LS_PHASES[int(r["phase"])]
        return r

    def lbfgs_update(self):
        """One L-BFGS iteration behind step_backward() (or the engine's mse begin phase), in place of step_update()."""
        self._chk(self.lib.gpe_lbfgs_update(self._h))

    def lbfgs_run(self, n_iters: int, mse: bool = False):
        """n_iters iterations "evaluate, iterate" enqueued back to back; no host synchronisation.  mse: the pre-training loss
        (bind_target).  With a line search n_iters counts evaluations ("evaluate, tick").  The monitor and the keeper are served
        after lbfgs_monitor(True), at the judged point (lbfgs_point) only."""
        self._chk(self.lib.gpe_lbfgs_run(self._h, int(n_iters), 1 if mse else 0))

    def lbfgs_monitor(self, on: bool = True):
        """Opt in (or out): every tick of lbfgs_run counts as one step of the bound monitor's `every`, and a monitor tick records -- and a
        bound keeper judges and keeps -- the JUDGED POINT: the parameters as they stand without a line search or once frozen, the start
        point of the running search (the last accepted point) under strong Wolfe.  The run itself goes on from the same bits.  The
        keeper's patience freezes the run for good with frozen code 4 ("keeper"), the parameters at the judged point of that record."""
        self._chk(self.lib.gpe_lbfgs_monitor(self._h, 1 if on else 0))

    def lbfgs_point(self) -> np.ndarray:
        """The judged point (see lbfgs_monitor) as get_params() would give it; synchronises, writes nothing on the device."""
        out = np.empty(self.n_params, np.float32)
        self._chk(self.lib.gpe_lbfgs_point(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def lbfgs_read(self) -> dict:
        """The last iteration's record and the state as it stands (LBFGS_FIELDS); `frozen` is a code: LBFGS_FROZEN[code] names it
        (0 live, 1 tolerance_grad, 2 nonfinite, 3 stop_loss, 4 keeper: the keeper's patience, lbfgs_monitor); synchronises."""
        out = (C.c_double * 16)()
        self._chk(self.lib.gpe_lbfgs_read(self._h, out))
        r = dict(zip(self.LBFGS_FIELDS, out))
        for k in ("n_iter", "count", "frozen", "skipped", "pushed", "head"):
            r[k] = int(r[k])
        return r

    def lbfgs_history(self):
        """(S, Y, g_prev, d): the pairs held, oldest first ([count, P]), the previous gradient and the direction ([P]); fp32."""
        m, P = getattr(self, "_lbfgs_history", 0), self.n_params
        S = np.zeros((max(m, 1), P), np.float32)
        Y = np.zeros((max(m, 1), P), np.float32)
        gp, d = np.zeros(P, np.float32), np.zeros(P, np.float32)
        n = C.c_int()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.gpe_lbfgs_history(self._h, vp(S), vp(Y), vp(gp), vp(d), P, C.byref(n)))
        return S[:n.value].copy(), Y[:n.value].copy(), gp, d

    # ---- continuation knobs --------------------------------------------------------------------------------------------
    def set_gamma(self, g: float):
        self.cfg.gamma = float(g)
        self._chk(self.lib.gpe_set_gamma(self._h, float(g)))

    def set_mixture(self, g11: float, g22: float, g12: float):
        """Coupling matrix of a mixture engine from the next step on (gamma-continuation)."""
        self._chk(self.lib.gpe_set_mixture(self._h, float(g11), float(g22), float(g12)))
        self.cfg.mix_g = (float(g11), float(g22), float(g12))

    MIXTURE_FIELDS = ("mu1", "mu2", "integral1", "integral2", "num1", "den1", "num2", "den2")

    def mixture_scalars(self) -> dict:
        """Both components' chemical potential, norm integral and Rayleigh sums of the last completed step (or residual()); synchronises."""
        out = (C.c_double * 8)()
        self._chk(self.lib.gpe_mixture_scalars(self._h, out))
        return dict(zip(self.MIXTURE_FIELDS, [float(v) for v in out]))

    MIXTURE_ENERGY_FIELDS = ("E", "T1", "T2", "Q11", "Q22", "Q12", "den1", "den2")

    def set_mixture_energy(self, w: float):
        """Weight w_E >= 0 of the mixture energy term from the next step on (include/gpe_hip.h: gpe_mixture_energy_weight): the loss gains
        w_E E, E the energy of the state normalised to the target norms, and the step's record reports E as 'riesz'.  0 switches it off."""
        self._chk(self.lib.gpe_mixture_energy_weight(self._h, float(w)))
        self.mixture_energy_weight = float(w)

    def mixture_energy(self) -> dict:
        """E and the sums it is formed from (T_a, Q_ab, den_a) on the bound set at the current parameters, at any weight; forward-only,
        synchronises, leaves parameters, optimiser state and the last record alone."""
        out = (C.c_double * 8)()
        self._chk(self.lib.gpe_mixture_energy(self._h, out))
        return dict(zip(self.MIXTURE_ENERGY_FIELDS, [float(v) for v in out]))

    def set_power(self, p: int):
        self.cfg.p = int(p)
        self._chk(self.lib.gpe_set_power(self._h, int(p)))

    def set_lr(self, lr: float):
        self._chk(self.lib.gpe_set_lr(self._h, float(lr)))

    def set_perturb_scale(self, s: float):
        self.cfg.perturb_scale = float(s)
        self._chk(self.lib.gpe_set_perturb_scale(self._h, float(s)))

    def set_loss_weights(self, w_pde, w_bc, w_norm, w_sym=0.0, w_orth=0.0, w_riesz=0.0):
        """Change the loss weights between steps (what a host-side balancer such as ReLoBRaLo needs)."""
        w = (C.c_float * 6)(w_pde, w_bc, w_norm, w_sym, w_orth, w_riesz)
        self._chk(self.lib.gpe_set_loss_weights(self._h, w))
        self.cfg.w_pde, self.cfg.w_bc, self.cfg.w_norm = float(w_pde), float(w_bc), float(w_norm)
        self.cfg.w_sym, self.cfg.w_orth, self.cfg.w_riesz = float(w_sym), float(w_orth), float(w_riesz)

    def set_n_global(self, n: int):
        self.cfg.n_global = int(n)
        self._chk(self.lib.gpe_set_n_global(self._h, int(n)))

    def profile_enable(self, on: bool = True):
        self._chk(self.lib.gpe_profile_enable(self._h, int(on)))

    def profile_read(self):
        """-> dict(fwd_ms, fwd_launches, bwd_ms, bwd_launches) measured with HIP events on the engine stream."""
        out = (C.c_double * 4)()
        self._chk(self.lib.gpe_profile_read(self._h, out))
        return dict(fwd_ms=out[0], fwd_launches=int(out[1]), bwd_ms=out[2], bwd_launches=int(out[3]))

    def step_cost(self):
        f, b = C.c_double(), C.c_double()
        self._chk(self.lib.gpe_step_cost(self._h, C.byref(f), C.byref(b)))
        return f.value, b.value
