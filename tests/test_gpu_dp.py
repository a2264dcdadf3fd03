"""world_size = 2 and 8 on ONE MI355X: one process per rank, each with its own HIP engine on cuda:0 and its block of the collocation
points, exchange the two step buffers with torch.distributed (gloo backend: NCCL/RCCL refuses two ranks on one device; the
data-parallel protocol and the engine's three-phase API are exactly what bench.py runs over RCCL).  The result must equal
the single-engine step on all points, and the fp64 oracle's at the tolerances of test_step_matches_oracle."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _case():
    rng = np.random.default_rng(11)
    layers = [2, 64, 64, 64, 1]
    N = 6001                                         # odd: ragged shards, last tile partial
    x = rng.uniform(-3, 3, (N, 2)).astype(np.float32)
    xb = rng.uniform(-3, 3, (9, 2)).astype(np.float32)
    P = sum(layers[i] * layers[i + 1] + layers[i + 1] for i in range(len(layers) - 1))
    flat = (rng.normal(0, 0.3, P)).astype(np.float32)
    kw = dict(layers=layers, gamma=40.0, dx=0.006, lr=1e-3, n_global=N)
    return kw, x, xb, flat


def _worker(rank, world, port, steps, out):
    from datetime import timedelta
    import torch.distributed as dist
    import gpe_pinn
    from gpe_pinn.dp import shard_points
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    # (a rank that dies ends its peers within the timeout instead of leaving them in all_reduce until the pytest limit)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    torch.cuda.set_device(0)
    kw, x, xb, flat = _case()
    eng = gpe_pinn.Engine(gpe_pinn.GPEConfig(**kw, world_size=world), device=0)
    eng.set_params(flat)
    eng.bind_points(torch.as_tensor(shard_points(x, rank, world), device="cuda:0"))
    eng.bind_boundary(torch.as_tensor(xb, device="cuda:0"))
    trace = []
    for k in range(steps):
        trace.append(eng.step_distributed(sync=True))
        if k == 0:
            grad1, flat1 = eng.get_grad(), eng.get_params()
    if rank == 0:
        np.savez(out, flat=eng.get_params(), loss=[t["loss"] for t in trace], mu=[t["mu"] for t in trace],
                 gn=[t["grad_norm"] for t in trace], bc=[t["bc"] for t in trace], pde=[t["pde"] for t in trace],
                 norm=[t["norm"] for t in trace], grad1=grad1, flat1=flat1)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 8])
def test_two_ranks_one_gpu_equal_single_engine(tmp_path, world):
    import torch.multiprocessing as mp
    import gpe_pinn
    from oracle import gpe_oracle as go
    from tests import helpers as H
    steps = 3
    out = str(tmp_path / "dp_gpu.npz")
    mp.get_context("spawn")
    mp.spawn(_worker, args=(world, _free_port(), steps, out), nprocs=world, join=True)
    got = np.load(out)
    kw, x, xb, flat = _case()
    eng = gpe_pinn.Engine(gpe_pinn.GPEConfig(**kw))
    eng.set_params(flat)
    eng.bind_points(torch.as_tensor(x, device="cuda"))
    eng.bind_boundary(torch.as_tensor(xb, device="cuda"))
    ref = [eng.step() for _ in range(steps)]
    np.testing.assert_allclose(got["loss"], [t["loss"] for t in ref], rtol=2e-5)
    np.testing.assert_allclose(got["mu"], [t["mu"] for t in ref], rtol=2e-6)
    np.testing.assert_allclose(got["gn"], [t["grad_norm"] for t in ref], rtol=2e-5)
    assert np.abs(got["flat"] - eng.get_params()).max() < 2e-5
    # ... and the fp64 oracle on all points: first step at the bounds of test_step_matches_oracle, the losses of all steps at the
    # trajectory bound of tools/fuzz_parity.py
    pb = go.Problem(layers=kw["layers"], gamma=kw["gamma"], dx=kw["dx"], n_global=kw["n_global"])
    x64, xb64, f64 = x.astype(np.float64), xb.astype(np.float64), flat.astype(np.float64)
    osc, ograd, _ = go.full_loss_and_grad(pb, f64, x64, xb64)
    for k, tol in (("mu", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("bc", 1e-4), ("norm", 2e-4)):
        assert abs(got[k][0] - osc[k]) <= tol * max(abs(osc[k]), 1e-6), (k, got[k][0], osc[k])
    assert abs(got["gn"][0] - np.linalg.norm(ograd)) < 1e-4 * np.linalg.norm(ograd)
    assert H.rel_err(got["grad1"], ograd) < 5e-5
    worst = H.block_rel_errs(got["grad1"], ograd, H.param_blocks(pb.layers))
    assert max(worst.values()) < 5e-5, worst
    new, _, _ = go.optimizer_step(go.OptState(lr0=kw["lr"]), flat, ograd, osc["loss"])
    d = np.abs(got["flat1"] - new)
    assert np.quantile(d, 0.99) < 2e-5 and d.max() < 2.1e-3
    _, tr = go.train_steps(pb, go.OptState(lr0=kw["lr"]), f64, x64, steps, xb64, dtype=np.float64)
    assert max(abs(a - t["loss"]) / abs(t["loss"]) / (1 + k) for k, (a, t) in enumerate(zip(got["loss"], tr))) < 1e-3


def _worker_native(rank, world, port, steps, out, stale):
    """One rank per GPU: torch.distributed(nccl) only for the rendezvous of the ncclUniqueId; both exchanges of a step by the engine's own
    RCCL communicator (gpe_comm_init / gpe_run_dp)."""
    import torch.distributed as dist
    import gpe_pinn
    from gpe_pinn.dp import shard_points
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    kw, x, xb, flat = _case()
    eng = gpe_pinn.Engine(gpe_pinn.GPEConfig(**kw, world_size=world), device=rank)
    eng.set_params(flat)
    eng.bind_points(torch.as_tensor(shard_points(x, rank, world), device=f"cuda:{rank}"))
    eng.bind_boundary(torch.as_tensor(xb, device=f"cuda:{rank}"))
    eng.comm_init(rank, world)
    if stale:
        eng.comm_set_async(True)
    trace = []
    for _ in range(steps):
        eng.run_dp(1)
        eng.synchronize()
        trace.append(eng.read_scalars())
    info = eng.comm_info()
    flats = [None] * world
    dist.all_gather_object(flats, eng.get_params())
    if rank == 0:
        np.savez(out, flat=flats[0], spread=max(float(np.abs(f - flats[0]).max()) for f in flats), loss=[t["loss"] for t in trace],
                 mu=[t["mu"] for t in trace], gn=[t["grad_norm"] for t in trace], world=info["world"], collectives=info["collectives"])
    dist.barrier()
    eng.close()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="the engine-native RCCL exchange at world > 1 needs two GPUs (RCCL refuses two ranks on one device)")
def test_native_rccl_two_ranks_equal_single_engine(tmp_path):
    """gpe_comm_init / gpe_step_dp with a real peer -- the ncclUniqueId rendezvous, both all-reduces on the exchange
    stream, the 1/world scaling of the replicated boundary batch -- against the single-engine trajectory on all points; replicas stay
    bit-identical.  Runs wherever two GPUs are visible (the build's boxes have one: skipped there, exercised by the driver's
    multi-GPU tier; bench.py cross-checks the same thing before timing at N > 1)."""
    import torch.multiprocessing as mp
    import gpe_pinn
    steps, world = 3, 2
    out = str(tmp_path / "dp_native.npz")
    mp.spawn(_worker_native, args=(world, _free_port(), steps, out, False), nprocs=world, join=True)
    got = np.load(out)
    assert int(got["world"]) == 2 and int(got["collectives"]) == 2 * steps and float(got["spread"]) == 0.0
    kw, x, xb, flat = _case()
    eng = gpe_pinn.Engine(gpe_pinn.GPEConfig(**kw))
    eng.set_params(flat)
    eng.bind_points(torch.as_tensor(x, device="cuda"))
    eng.bind_boundary(torch.as_tensor(xb, device="cuda"))
    ref = [eng.step() for _ in range(steps)]
    np.testing.assert_allclose(got["loss"], [t["loss"] for t in ref], rtol=2e-5)
    np.testing.assert_allclose(got["mu"], [t["mu"] for t in ref], rtol=2e-6)
    np.testing.assert_allclose(got["gn"], [t["grad_norm"] for t in ref], rtol=2e-5)
    assert np.abs(got["flat"] - eng.get_params()).max() < 2e-5
