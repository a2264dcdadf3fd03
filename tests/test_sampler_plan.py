"""The host-only part of a sampler bind (csrc/gpe_sampler_plan.h: sampler_plan) under the address and undefined-behaviour sanitizers.
tests/sampler_plan_selftest.cpp includes that header alone; it is built here with g++ -fsanitize=address,undefined and run as a child
process on a file of cases -- no GPU, nothing loaded into Python.  Every caller array in it is a heap block of exactly its length, so a
read past edges[k][shape[k]] or past cells[n - 1] ends the child with a report.

Refusals: the codes and the substrings tests/test_gpu_sampler_cells.py (_refusals), test_gpu_sampler.py, test_gpu_weights.py and
test_gpu_adaptive_sampler.py assert on a live engine.  Accepted inputs: n_rows, n_edges, W and the block volumes, compared for equality
with gpe_pinn.sampler (graded_total, cells_total, graded_weights) and the counts the spec implies."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gpe_pinn import capi
from gpe_pinn import sampler as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sampler_plan_selftest.cpp")

GRID = {1: dict(lo=(-6.0,), hi=(6.0,), shape=(16,)),
        2: dict(lo=(-3.0, -2.5), hi=(3.0, 2.5), shape=(12, 10)),
        3: dict(lo=(-3.0, -2.5, -2.0), hi=(3.0, 2.5, 2.0), shape=(6, 5, 4))}
EDGES = {1: [S.sinh_edges(6.0, 16, 2.0)], 2: [S.sinh_edges(3.0, 12, 2.5), S.sinh_edges(2.5, 10, 1.0)],
         3: [S.sinh_edges(3.0, 6, 1.5), S.sinh_edges(2.5, 5, 2.0), S.sinh_edges(2.0, 4, 0.5)]}
LIST = {1: np.array([0, 1, 5, 6, 7, 15], dtype=np.int64), 2: S.ball_cells(radius=2.0, **GRID[2]), 3: S.ball_cells(radius=2.0, **GRID[3])}
DISK = LIST[2]
BLOCKS = {1: [S.sinh_edges(6.0, 8, 2.0)], 2: [S.sinh_edges(3.0, 4, 2.0), S.sinh_edges(2.5, 3, 1.0)],
          3: [S.sinh_edges(3.0, 3, 1.5), S.sinh_edges(2.5, 2, 2.0), S.sinh_edges(2.0, 2, 0.5)]}


def fhex(v):
    return float(np.float32(v)).hex()


def case(name, dim=2, w_sym=False, shape=None, lo=None, hi=None, clip=None, first=0, n_local=None, every=3, edges=None, ad=None, cells=None):
    """one case of the child's input; edges: None, or one array (or None: a NULL pointer) per axis; ad: (n_points, n_min, uniform_per_1024)"""
    g = GRID[dim]
    shape = g["shape"] if shape is None else shape
    lo, hi = g["lo"] if lo is None else lo, g["hi"] if hi is None else hi
    clo, chi = (lo, hi) if clip is None else clip
    total = 1
    for s in shape:
        total *= s
    if n_local is None:
        n_local = (total if cells is None else len(cells)) - first
    pad = lambda v, fill: list(v) + [fill] * (3 - len(v))
    t = ["case", name, "dim", dim, "wsym", int(w_sym), "shape", *pad(shape, 0)]
    for key, v in (("lo", lo), ("hi", hi), ("clip_lo", clo), ("clip_hi", chi)):
        t += [key, *[fhex(x) for x in pad(v, 0.0)]]
    t += ["first", first, "n_local", n_local, "every", every]
    if edges is None:
        t += ["edges", 0]
    else:
        t += ["edges", 1]
        for a in pad(edges, None):
            t += [0] if a is None else [len(a), *[fhex(x) for x in a]]
    t += ["ad", 0] if ad is None else ["ad", 1, *ad]
    t += ["cells", 0] if cells is None else ["cells", 1, len(cells), *[int(c) for c in cells]]
    return " ".join(str(x) for x in t)


def refusals():
    """name -> (case, the message's first word, a substring of the message)"""
    e0, e1 = EDGES[2]
    flat_edge = e0.copy(); flat_edge[3] = flat_edge[2]
    nan_edge = e0.copy(); nan_edge[2] = np.nan
    short_edge = e0[:-1].copy()                          # one entry fewer than shape[0] + 1: its last value is not hi
    R = {}
    # tests/test_gpu_sampler_cells.py: _refusals (the three the entry point judges before the plan, on n_cells and a NULL list, are not the plan's)
    cl = lambda name, text, **kw: R.__setitem__("cells " + name, (case("cells_" + name.replace(" ", "_").replace(",", ""), **kw), "sampler_cells:", text))
    cl("not ascending", "position 2", cells=[0, 5, 5, 9])
    cl("descending", "position 3", cells=[0, 5, 9, 8, 7])
    cl("cell beyond the grid", "cells[2] = 120", cells=[0, 5, 120])
    cl("negative cell", "cells[0] = -1", cells=[-1, 5])
    cl("first < 0", "rows", cells=DISK, first=-1, n_local=5)
    cl("n_local = 0", "rows", cells=DISK, n_local=0)
    cl("rows beyond the list", "rows", cells=DISK, first=DISK.size - 2, n_local=3)
    cl("rows beyond the list, within the grid", "rows", cells=DISK, first=0, n_local=DISK.size + 1)
    cl("every = 0", "every", cells=DISK, every=0)
    cl("every < 0", "every", cells=DISK, every=-2)
    cl("hi <= lo", "hi <= lo", cells=DISK, hi=(3.0, -2.5))
    cl("one axis for two", "input axes", cells=[0, 1], shape=(120,), lo=(-3.0,), hi=(3.0,))
    cl("three axes for two", "input axes", cells=[0, 1], shape=(12, 5, 2), lo=(-3.0, -2.5, -1.0), hi=(3.0, 2.5, 1.0))
    cl("axis index beyond 2^24", "2^24", cells=[0, 1], shape=(2 ** 24 + 1, 10))
    cl("edges for one axis of two", "no edges for axis 1", cells=DISK, edges=(e0, None))
    cl("edges for the other axis", "no edges for axis 0", cells=DISK, edges=(None, e1))
    cl("edges that do not increase", "do not increase", cells=DISK, edges=(flat_edge, e1))
    cl("an edge that is not finite", "not finite", cells=DISK, edges=(nan_edge, e1))
    cl("lo other than the first edge", "first / last edge", cells=DISK, edges=(e0, e1), lo=(-2.5, -2.5))
    # A volume is formed only behind both scans.  cell_volume splits a cell with % and /, so a cell past the grid wraps to indices inside
    # it and reads nothing out of bounds: those cases hold the refusal's text alone.  A NEGATIVE cell gives a negative remainder on some
    # axis, and a volume formed ahead of the list scan would read edges[k][-1], in front of the heap block: the sanitizer's case.
    cl("graded, cell beyond the grid", "cells[2] = 120", cells=[0, 5, 120], edges=(e0, e1))
    cl("graded, last cell + 1", "cells[1] = 120", cells=[119, 120], edges=(e0, e1))
    cl("graded, negative first cell", "cells[0] = -1", cells=[-1, 5], edges=(e0, e1))
    cl("graded, negative cell behind a good one", "cells[1] = -7", cells=[0, -7], edges=(e0, e1))
    cl("graded, negative cell on the first axis only", "cells[0] = -20", cells=[-20, 3], edges=(e0, e1))
    cl("graded, edges that do not increase, last cell listed", "do not increase", cells=[0, 119], edges=(flat_edge, e1))
    cl("graded, symmetry batch", "w_sym", cells=DISK, edges=(e0, e1), w_sym=True)
    # the plain sampler (tests/test_gpu_sampler.py: test_specs_the_engine_cannot_honour_are_invalid, on a 20 x 20 grid)
    g = dict(lo=(-3.0, -3.0), hi=(3.0, 3.0), shape=(20, 20), every=5)
    pl = lambda name, text, **kw: R.__setitem__("plain " + name, (case("plain_" + name.replace(" ", "_"), **{**g, **kw}), "bind_sampler:", text))
    pl("every = 0", "every = 0", every=0)
    pl("every < 0", "every = -3", every=-3)
    pl("hi <= lo on axis 1", "hi <= lo on axis 1", hi=(3.0, -3.0))
    pl("hi <= lo on axis 0", "hi <= lo on axis 0", hi=(-3.0, 3.0))
    pl("clip_hi < clip_lo", "clip_hi < clip_lo on axis 1", clip=((0.0, 1.0), (1.0, 0.5)))
    pl("cells beyond the grid", "outside the grid's 400", first=399, n_local=2)
    pl("first < 0", "outside the grid's 400", first=-1, n_local=5)
    pl("n > cells", "outside the grid's 400", n_local=401)
    pl("one axis for two", "input axes", lo=(-3.0,), hi=(3.0,), shape=(400,))
    pl("three axes for two", "input axes", lo=(-3.0,) * 3, hi=(3.0,) * 3, shape=(20, 5, 4))
    # the graded sampler (tests/test_gpu_weights.py)
    gr = lambda name, text, **kw: R.__setitem__("graded " + name, (case("graded_" + name.replace(" ", "_"), **kw), "bind_sampler_graded:", text))
    gr("edges that do not increase", "do not increase at 3", edges=(flat_edge, e1))
    gr("an edge that is not finite", "edge 2 of axis 0 is not finite", edges=(nan_edge, e1))
    gr("no edges for axis 1", "no edges for axis 1", edges=(e0, None))
    gr("lo other than the first edge", "first / last edge", edges=(e0, e1), lo=(-2.5, -2.5))
    gr("hi other than the last edge", "first / last edge", edges=(e0, e1), hi=(3.0, 2.0))
    gr("one edge too few", "first / last edge", edges=(short_edge, e1), shape=(11, 10))
    gr("symmetry batch", "w_sym", edges=(e0, e1), w_sym=True)
    gr("every before the symmetry batch", "every = 0", edges=(e0, e1), w_sym=True, every=0)
    gr("cells beyond the grid", "outside the grid's 120", edges=(e0, e1), first=100, n_local=21)
    # the adaptive sampler (tests/test_gpu_adaptive_sampler.py: test_refusals_and_lifetime)
    b0, b1 = BLOCKS[2]
    B = 12
    tiny = [np.array([0.0, 1e-30, 2e-30], np.float32), np.array([0.0, 1e-30], np.float32)]      # 2 blocks of volume 1e-60: 0 in fp32
    ad = lambda name, text, **kw: R.__setitem__("adaptive " + name, (case("adaptive_" + name.replace(" ", "_"), **{**dict(
        shape=(4, 3), edges=(b0, b1), ad=(96, 2, 512)), **kw}), "sampler_adaptive:", text))
    ad("n_points > 2^22", "n_points = 4194305", ad=((1 << 22) + 1, 2, 512))
    ad("n_points = 0", "n_points = 0", ad=(0, 2, 512))
    ad("blocks do not fit", "do not fit 23 points", ad=(B * 2 - 1, 2, 512))
    ad("n_min = 0", "n_min = 0", ad=(96, 0, 512))
    ad("uniform_per_1024 = 0", "uniform_per_1024 = 0", ad=(96, 2, 0))
    ad("uniform_per_1024 = 1025", "uniform_per_1024 = 1025", ad=(96, 2, 1025))
    ad("a block of the cells", "single-rank", first=0, n_local=B - 1)
    ad("first_cell != 0", "single-rank", first=1, n_local=B - 1)
    ad("every = 0", "every = 0", every=0)
    ad("clip_hi < clip_lo", "clip_hi < clip_lo", clip=((1.0, 1.0), (0.0, 0.0)))
    ad("edges that do not increase", "do not increase", edges=(np.array([-3.0, -1.0, -1.0, 1.0, 3.0], np.float32), b1))
    ad("no edges for axis 1", "no edges for axis 1", edges=(b0, None))
    ad("symmetry batch", "w_sym", w_sym=True)
    ad("volume underflow", "underflow or overflow fp32", shape=(2, 1), lo=(0.0, 0.0), hi=(2e-30, 1e-30), edges=tiny, ad=(8, 1, 512))
    return R


def accepted():
    """name -> (case, n_rows, n_edges, W, block volumes)"""
    A = {}
    for d in (1, 2, 3):
        g, ed, cells, bl = GRID[d], EDGES[d], LIST[d], BLOCKS[d]
        total = int(np.prod(g["shape"]))
        n_edges = sum(a.size for a in ed)
        ends = dict(lo=[a[0] for a in ed], hi=[a[-1] for a in ed])
        none = np.zeros(0, np.float32)
        A[f"uniform {d}d"] = (case(f"uniform_{d}d", dim=d), total, 0, 1.0, none)
        A[f"uniform {d}d, a block"] = (case(f"uniform_{d}d_block", dim=d, first=3, n_local=total - 5), total - 5, 0, 1.0, none)
        A[f"graded {d}d"] = (case(f"graded_{d}d", dim=d, edges=ed, **ends), total, n_edges, S.graded_total(ed), none)
        A[f"graded {d}d, a block"] = (case(f"graded_{d}d_block", dim=d, edges=ed, first=2, n_local=7, **ends), 7, n_edges, S.graded_total(ed), none)
        A[f"list {d}d"] = (case(f"list_{d}d", dim=d, cells=cells), cells.size, 0, 1.0, none)
        A[f"graded list {d}d"] = (case(f"graded_list_{d}d", dim=d, cells=cells, edges=ed, **ends), cells.size, n_edges, S.cells_total(cells, ed), none)
        A[f"graded list {d}d, rows 1 .. 3"] = (case(f"graded_list_{d}d_rows", dim=d, cells=cells, edges=ed, first=1, n_local=3, **ends), 3, n_edges,
                                              S.cells_total(cells, ed), none)
        A[f"graded list {d}d, the last cell"] = (case(f"graded_list_{d}d_last", dim=d, cells=[total - 1], edges=ed, **ends), 1, n_edges,
                                                S.cells_total([total - 1], ed), none)
        shape = tuple(a.size - 1 for a in bl)
        B = int(np.prod(shape))
        A[f"adaptive {d}d"] = (case(f"adaptive_{d}d", dim=d, shape=shape, edges=bl, ad=(7 * B + 3, 2, 256), lo=[a[0] for a in bl], hi=[a[-1] for a in bl]),
                               7 * B + 3, sum(a.size for a in bl), S.graded_total(bl), S.graded_weights(bl))
    return A


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """the child's stdout lines by case name, from one sanitizer build and one run over every case"""
    if shutil.which("g++") is None:
        pytest.fail("no g++ on this host: the plan's sanitizer self-test cannot be built")
    tmp = tmp_path_factory.mktemp("sampler_plan")
    exe, cases = str(tmp / "sampler_plan_selftest"), str(tmp / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, SRC])
    lines = [c[0] for c in refusals().values()] + [c[0] for c in accepted().values()]
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, "sanitizer self-test failed:\n" + out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert got[-1] == f"done {len(lines)}", got[-1]
    return {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in got[:-1]}


def test_every_refusal_has_its_code_and_text(child):
    R = refusals()
    assert len(R) == 59
    for name, (text, who, sub) in R.items():
        got = child[text.split()[1]]
        verdict, code, msg = got.split(" ", 2)
        assert verdict == "refused" and int(code) == capi.GPE_ERR_INVALID and msg.startswith(who) and sub in msg, (name, got)


def test_accepted_inputs_give_the_counts_and_volumes_of_the_numpy_restatement(child):
    for name, (text, n_rows, n_edges, W, vol) in accepted().items():
        t = child[text.split()[1]].split()
        assert t[0] == "ok" and t[1::2][:4] == ["n_rows", "n_edges", "w_grid", "vol"], (name, t)
        assert (int(t[2]), int(t[4])) == (n_rows, n_edges), (name, t[:6])
        assert float.fromhex(t[6]) == W, (name, t[6], float(W).hex())
        got = np.array([float.fromhex(v) for v in t[9:]], dtype=np.float64)
        assert int(t[8]) == vol.size == got.size and np.array_equal(got, vol.astype(np.float64)), (name, got, vol)
