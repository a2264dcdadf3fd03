"""The default kernel selection on both sides of every batch-size seam (tests/seam_table.py), at the real sizes.

Discovery: per class one engine is rebound along a ladder of sizes and every interval whose ends report different active_kernels
is bisected; each change must land on a visible row of the table, and each visible row must be found.

Cells: (class, seam) -> both sizes, lower | lower + 1 (the upper batch's last tile holds one point, a merged boundary point),
each against the fp64 oracle: forward_jets, residual(), one step with the bounds of test_step_matches_oracle, the gradient per
parameter block at 5e-5 of the block's own maximum, the parameters after Adam, and the active_kernels strings the rows promise.
Across the seam mu and loss may differ by what the oracle's two values differ plus those bounds.  Further cells: run(8) against
eight step() calls at the graph-replay limit, two engines bit for bit where the README promises it, and weights of ones on both
sides of both head seams.

Sizes are launched points (bound + 5 merged boundary points) unless the row counts collocation points.  With SEAMS_REPORT naming a
file, the module leaves the per-cell figures there when its last test is done; tools/seam_figures.py puts the oracle's float32
figures beside them (profiles/seams/seams_time.txt).

Measured on the MI355X (256 CUs; profiles/seams/seams_time.txt has every cell, with the oracle's float32 figures beside): the module
takes 64 s, fp64 references included; the slowest test is g512 at 16 635 | 16 636 bound points, 8.9 s, nearly all of it the two
references.  Largest relative errors against the oracle over all 74 cells (records, not bounds): mu 1.5e-7 (w256, 2 044), loss 5.5e-7
(gres, 124), gradient 1.7e-6 whole (gres, 131 099), 1.0e-5 worst block (g512, 251: the generic set's split-K sums, a fifth of the
bound); no side of any seam stands out.
"""
import json
import os
import time

import numpy as np
import pytest
import torch

import gpe_pinn
from gpe_pinn import Engine
from oracle import gpe_oracle as go
from tests import helpers as H
from tests import seam_ref as R
from tests import seam_table as S
from tests.test_gpu_parity import cfg_from_problem, close

pytestmark = pytest.mark.gpu

LADDER_TOP = 600000
RECORDS = {}


@pytest.fixture(scope="module", autouse=True)
def seam_figures():
    """the per-cell figures of this run, written where SEAMS_REPORT points once the module's tests are done"""
    yield
    out = os.environ.get("SEAMS_REPORT")
    if out and RECORDS:
        with open(out, "w") as f:
            json.dump(RECORDS, f, indent=1)


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def kstr(k):
    return ";".join(f"{a}={b}" for a, b in k.items())


def make(cls, n, weights=False):
    x, flat, x_bc = S.inputs(cls, n)
    eng = Engine(cfg_from_problem(R.problem(cls)))
    eng.set_params(flat)
    eng.bind_points(torch.as_tensor(x, device="cuda"))
    eng.bind_boundary(torch.as_tensor(x_bc, device="cuda"))
    if weights:
        eng.bind_weights(torch.ones(n, device="cuda"))
    return eng


# ---- discovery ------------------------------------------------------------------------------------------------------------------------
def ladder(top=LADDER_TOP, first=1):
    pts = set()
    p = first
    while p <= top:
        for b in (p, p + p // 2):
            pts |= {m for m in (b - 1, b, b + 1) if first <= m <= top}
        p *= 2
    return sorted(pts | {top})


@pytest.mark.parametrize("cls", sorted(S.CLASSES))
def test_every_change_of_active_kernels_is_a_row_of_the_table(cls):
    cu = cu_count()
    x, flat, x_bc = S.inputs(cls, LADDER_TOP)
    xd = torch.as_tensor(x, device="cuda")
    eng = Engine(cfg_from_problem(R.problem(cls)))
    eng.set_params(flat)
    eng.bind_points(xd[:1])
    eng.bind_boundary(torch.as_tensor(x_bc, device="cuda"))
    seen = {}

    def k(n):
        if n not in seen:
            eng.bind_points(xd[:n])              # (bind only: the names are a function of what is bound)
            seen[n] = kstr(eng.active_kernels)
        return seen[n]

    found = {}

    def bisect(a, b):
        if k(a) == k(b):
            return
        if b == a + 1:
            found[a] = (k(a), k(b))
            return
        m = (a + b) // 2
        bisect(a, m)
        bisect(m, b)

    lad = ladder()
    for a, b in zip(lad[:-1], lad[1:]):
        bisect(a, b)
    eng.close()
    want = {n: names for n, names in S.class_seams(cls, cu) if any(S.SEAMS[r]["visible"] for r in names) and n < LADDER_TOP}
    extra = {n: v for n, v in found.items() if n not in want}
    missed = {n: v for n, v in want.items() if n not in found}
    assert not extra, f"{cls}: active_kernels changes at sizes the seam table has no visible row for (bound points n | n + 1): {extra}"
    assert not missed, f"{cls}: visible rows not found by the ladder: {missed}"
    for n in found:
        for m in (n, n + 1):
            bad = S.mismatches(dict(kv.split("=", 1) for kv in k(m).split(";")), S.expected(cls, m, cu))
            assert not bad, (cls, m, bad)


# ---- both sides against the oracle ------------------------------------------------------------------------------------------------------
_CELL = {}


def cell(cls, n, weights=False):
    """one size: the engine's step against the oracle's; -> dict(bad, kern, sc, osc)"""
    key = (cls, n, weights)
    if key in _CELL:
        return _CELL[key]
    t0 = time.time()
    pb = R.problem(cls)
    x, flat, x_bc = S.inputs(cls, n)
    osc, ograd = R.step(cls, n)
    ojets, opsi, ores = R.fields(cls, n, osc["mu"])
    new, _, _ = go.optimizer_step(go.OptState(lr0=1e-3), flat, ograd, osc["loss"])
    t_ref = time.time() - t0
    bad = []
    eng = make(cls, n, weights)
    try:
        kern = eng.active_kernels
        if eng.active_path != (gpe_pinn.PATH_GENERIC if S.CLASSES[cls][1]["path"] == "generic" else gpe_pinn.PATH_FUSED):
            bad.append(f"kernel set {eng.active_path} is not the table's {S.CLASSES[cls][1]['path']}")
        jets = eng.forward_jets(torch.as_tensor(x, device="cuda")).cpu().numpy()
        for c in range(jets.shape[0]):
            if not close(jets[c], ojets[c], 1e-5, 2e-6):
                bad.append(f"jet channel {c}: err {np.abs(jets[c] - ojets[c]).max():.3e}")
        rs, psi, res = eng.residual()
        if not close(psi.cpu().numpy(), opsi, 5e-6, 2e-6):
            bad.append("residual(): psi")
        if not close(res.cpu().numpy(), ores, 2e-5, 1e-5):
            bad.append("residual(): residual")
        if abs(rs["loss"] - osc["loss"]) > 1e-4 * abs(osc["loss"]):
            bad.append(f"residual(): loss {rs['loss']:.9g} vs {osc['loss']:.9g}")
        sc = eng.step()
        grad = eng.get_grad()
        params = eng.get_params()
    finally:
        eng.close()
    rec = {}
    for kk, tol in (("mu", 2e-5), ("loss", 1e-4), ("pde", 1e-4), ("bc", 1e-4), ("norm", 2e-4)):
        rec[kk] = abs(sc[kk] - osc[kk]) / max(abs(osc[kk]), 1e-6)
        if rec[kk] > tol:
            bad.append(f"{kk} {sc[kk]:.9g} vs oracle {osc[kk]:.9g}")
    rec["grad"] = H.rel_err(grad, ograd)
    if not rec["grad"] < 5e-5:
        bad.append(f"gradient rel err {rec['grad']:.3e}")
    rec["block"] = max(H.block_rel_errs(grad, ograd, H.param_blocks(pb.layers, pb.net_kind)).values())
    bad += H.block_failures(grad, ograd, pb.layers, pb.net_kind)
    gn = np.linalg.norm(ograd)
    if abs(sc["grad_norm"] - gn) > 1e-4 * gn:
        bad.append(f"grad_norm {sc['grad_norm']:.9g} vs {gn:.9g}")
    d = np.abs(params - new)
    if not (np.quantile(d, 0.99) < 2e-5 and d.max() < 2.1e-3):
        bad.append(f"parameters after Adam: q99 {np.quantile(d, 0.99):.3e} max {d.max():.3e}")
    rec.update(kernels=kstr(kern), seconds=time.time() - t0, reference_seconds=t_ref)
    RECORDS[f"{cls}-{n}{'-weighted' if weights else ''}"] = rec
    tag = f"[{cls} {n} bound points -> {kstr(kern)}]"
    _CELL[key] = dict(bad=[f"{tag} {m}" for m in bad], kern=kern, sc=sc, osc=osc, grad=grad)
    return _CELL[key]


PAIRS = [(cls, row) for row in S.SEAMS if S.SEAMS[row]["counts"] != "obs" for cls in S.SEAMS[row]["cells"]]


@pytest.mark.parametrize("cls,row", PAIRS, ids=[f"{c}-{r}" for c, r in PAIRS])
def test_both_sides_of_the_seam_match_the_oracle(cls, row):
    cu = cu_count()
    n = S.bound_n(S.SEAMS[row], cu)
    lo, hi = cell(cls, n), cell(cls, n + 1)
    bad = lo["bad"] + hi["bad"]
    for c, m in ((lo, n), (hi, n + 1)):
        bad += [f"[{cls} {m}] {s}" for s in S.mismatches(c["kern"], S.expected(cls, m, cu))]
    here = dict(S.class_seams(cls, cu))[n]
    if not any(S.SEAMS[r]["visible"] for r in here) and lo["kern"] != hi["kern"]:
        bad.append(f"[{cls} {n} | {n + 1}] names change across a seam no visible row is at: {kstr(lo['kern'])} | {kstr(hi['kern'])}")
    # one added point: the engine's two values differ by what the oracle's two differ, plus each side's own bound
    for kk, tol in (("mu", 2e-5), ("loss", 1e-4)):
        de, do = abs(lo["sc"][kk] - hi["sc"][kk]), abs(lo["osc"][kk] - hi["osc"][kk])
        if de > do + tol * (abs(lo["osc"][kk]) + abs(hi["osc"][kk])):
            bad.append(f"[{cls} {n} | {n + 1}] {kk} jumps by {de:.3e} across the seam, the oracle's by {do:.3e}")
    assert not bad, f"{len(bad)} failing checks\n" + "\n".join(bad)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("cls", ["A", "B"])
def test_graph_replay_limit_run_equals_steps(cls, side):
    """graph_max_points | + 1 launched points: step() + run(8) (replayed graphs | direct launches) and nine step() calls from one start
    give the same parameters bit for bit.  The loss history is held to 1e-12 relative and NOT bit for bit, on purpose: its sum of r^2 is
    added by double atomics in arrival order, which the README excepts from the bit-for-bit promise, so equal bits would be luck
    (1e-12: some 4 000 roundings of 2^-53 among up to 17 workgroup sums, with room).  Both follow the oracle's 9-step trajectory by the
    switch matrix's measure.  What this cannot see: gpe_run falls back to plain launches without a word when the capture fails, and
    the library exposes no count of replays, so the lower side proves only that whatever run(8) did equals eight steps."""
    n = S.bound_n(S.SEAMS["graph_max_points"], cu_count()) + side
    out = []
    for use_run in (True, False):
        eng = make(cls, n)
        eng.step()
        if use_run:
            eng.run(8)
        else:
            for _ in range(8):
                eng.step()
        out.append((np.array([h["loss"] for h in eng.read_history(1, 9)]), eng.get_params()))
        eng.close()
    assert np.array_equal(out[0][1], out[1][1]), f"{cls} {n}: parameters after run(8) differ from eight step() calls"
    assert np.abs(out[0][0] - out[1][0]).max() <= 1e-12 * np.abs(out[1][0]).max(), (out[0][0], out[1][0])
    x, flat, x_bc = S.inputs(cls, n)
    _, tr = go.train_steps(R.problem(cls), go.OptState(lr0=1e-3), flat.astype(np.float64), x.astype(np.float64), 9, x_bc.astype(np.float64),
                           dtype=np.float64)
    for losses, _ in out:
        dev = max(abs(a - t["loss"]) / max(abs(t["loss"]), 1e-30) / (1 + k) for k, (a, t) in enumerate(zip(losses, tr)))
        assert dev < 1e-3, f"{cls} {n}: 9-step loss trajectory off the oracle's: {dev:.3e}"


@pytest.mark.parametrize("cls", ["A", "NS"])
def test_two_engines_repeat_bit_for_bit_around_the_head_seams(cls):
    """head inside a forward kernel (<= fuse_head_max, >= fuse_head_tile_min launched points): mu, norm and gradient of two engines are
    the same bits; one point beyond either seam (k_head_pde: double atomics) the gradient still is"""
    cu = cu_count()
    a, b = S.bound_n(S.SEAMS["fuse_head_max"], cu), S.bound_n(S.SEAMS["fuse_head_tile_min"], cu)
    for n, fused in ((a, True), (a + 1, False), (b, False), (b + 1, True)):
        runs = []
        for _ in range(2):
            eng = make(cls, n)
            assert eng.active_kernels["fwd"].endswith(",head>") == fused, (n, eng.active_kernels)
            sc = eng.step()
            runs.append((sc["mu"], sc["norm"], eng.get_grad()))
            eng.close()
        assert np.array_equal(runs[0][2], runs[1][2]), f"{cls} {n}: gradient bits differ between two engines"
        if fused:
            assert runs[0][:2] == runs[1][:2], f"{cls} {n}: mu / norm bits differ: {runs[0][:2]} {runs[1][:2]}"


@pytest.mark.parametrize("row", ["fuse_head_max", "fuse_head_tile_min"])
def test_weights_of_ones_on_both_sides_of_the_head_seams(row):
    """bound weights keep head and seeds on the weighted k_head_pde / k_seed_pde whatever the size; ones give the unweighted step"""
    n = S.bound_n(S.SEAMS[row], cu_count())
    bad = []
    for m in (n, n + 1):
        c = cell("A", m, weights=True)
        k = c["kern"]
        bad += c["bad"]
        if not ("weighted" in k.get("head", "") and "weighted" in k.get("seed", "")):
            bad.append(f"[A {m}] no weighted head / seed entries: {kstr(k)}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("side", [0, 1])
def test_observables_and_monitor_at_the_reduction_grid_cap(side):
    """OBS_THREADS * OBS_MAX_WG | + 1 points handed to observables(): one point per thread | threads loop.  Every field against the fp64
    reference of tests/test_observables_cpu.py with the bounds of tests/test_gpu_observables.py; and the monitor on the same points
    after one step equals observables() asked then, byte for byte (the same launches)."""
    from tests.test_gpu_observables import check_against, oracle_jets, _bytes
    from tests.test_observables_cpu import observables_ref
    n = S.SEAMS["obs_grid_cap"]["lower"](cu_count()) + side
    pb = R.problem("A")
    x, flat, x_bc = S.inputs("A", n)
    x64 = x.astype(np.float64)
    ref, scale = observables_ref(pb, x64, go.head_pde(pb, x64, oracle_jets(pb, flat, x64)), pb.dx)
    xd = torch.as_tensor(x, device="cuda")
    eng = make("A", 4096)
    eng.set_params(flat)                        # (S.inputs draws the parameters behind the points: those of this size)
    try:
        check_against(eng.observables(xd), ref, scale, n, pb.dx)
        eng.bind_monitor(xd, every=1)
        eng.step()
        rec = eng.read_monitor()
        assert len(rec) == 1 and rec[0]["step"] == 1.0
        assert _bytes(rec[0]) == _bytes(eng.observables(xd))
    finally:
        eng.close()
