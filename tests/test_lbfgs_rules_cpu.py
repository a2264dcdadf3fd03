"""The scalar rules of the device-resident L-BFGS (csrc/gpe_lbfgs_rules.h: ls_decide, ls_rearm, ls_cubic, ls_free_slot, lbfgs_freeze,
lbfgs_judged_at_start) under the address and undefined-behaviour sanitizers, against tests/lbfgs_ls_ref.py.
tests/lbfgs_rules_selftest.cpp includes that header alone; it is built here with g++ -O1 -ffp-contract=off -fsanitize=address,undefined and
run as a child process on a trace -- no GPU, nothing loaded into Python.

The trace: the reference runs in fp64 on the small problems of tests/test_lbfgs_ls_reference_cpu.py, on the tick cases and end cells of
tests/lbfgs_ls_cases.py and on a few 1-D profiles and scripted losses below; per tick it logs what the machine is fed (loss, g.d, sum|g|,
max|g|, max|d|; hex floats) and, where it accepts a point, what the iteration hands back (freeze code, loss, g.d of the new direction, the
first step, the skip flag).  The child replays the inputs through the header and prints its state after every tick.  Both sides are IEEE
double, same operation order, no contraction: EVERY field is compared for equality, doubles included.

Before comparing, the reference's own records must show that the traces reach every exit of the machine (test_the_traces_reach_every_exit)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import lbfgs_ls_cases as cases
from tests import lbfgs_ls_ref as ls_
from tests.test_lbfgs_ls_reference_cpu import PROBLEMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "lbfgs_rules_selftest.cpp")
NONE, TRIAL, ACCEPT, RESTORE = 0, 1, 2, 3                # LS_ACT_*
EXITS = ("extrapolation", "extrapolation past a second trial that rose", "bracket by armijo", "bracket by loss >= bf[0]",
         "bracket by gtd >= 0", "curvature accept in bracket", "curvature accept in zoom", "max_ls fallback", "end by max_ls", "width break",
         "insufficient-progress nudge to the upper end", "insufficient-progress nudge to the lower end", "insufficient progress flagged",
         "accepted point is not the last", "stalled accept", "non-finite trial in bracket", "non-finite trial in zoom",
         "non-finite trial in zoom, low end off the start", "tick on a frozen state", "iteration froze", "iteration skipped",
         "evaluation at theta0")
NOT_ASKED = {"out-of-bracket nudge"}                     # a nudge with the flag down (the interpolant fell on or outside an end): named if met


def hx(v):
    return float(v).hex()


class Trace:
    """one run of the reference: the child's input lines, what the child must print per tick, and the exits each tick took"""
    def __init__(self, name, ref):
        self.name, self.ref = name, ref
        lb = ref.lb
        self.lines = [" ".join(["run", name, hx(lb.lr), hx(lb.tolerance_grad), hx(lb.tolerance_change), hx(lb.stop_loss), str(lb.history),
                                hx(ref.c1), hx(ref.c2), str(ref.max_ls)])]
        self.want, self.exits = [], []

    def tick(self, loss, g):
        ref, lb = self.ref, self.ref.lb
        g = np.asarray(g, np.float64)                    # (the reference takes this very array: its g.d is this g.d)
        with np.errstate(all="ignore"):
            gtd, g1, gmax, dmax = float(g @ lb.d), float(np.abs(g).sum()), float(np.abs(g).max()), float(np.abs(lb.d).max())
        pre = dict(frozen=lb.frozen, state=ref.state, insuf=ref.insuf, t=ref.t, ls_iter=ref.ls_iter, f0=ref.f0, gtd0=ref.gtd0, bf0=ref.bf[0],
                   t_low=ref.b[ref.low_pos], counts=(ref.end_curv, ref.end_max_ls, ref.end_width, ref.stalled))
        out = ref.tick(loss, g)
        self.lines.append(" ".join(["tick", hx(loss), hx(gtd), hx(g1), hx(gmax), hx(dmax)]))
        it = out["iteration"]
        if it is not None:
            froze = it["status"] == "frozen"
            self.lines.append(" ".join(["iter", str(it["frozen"]), hx(it["loss"]), hx(it["gtd"]), hx(it["t"]), str(int(it["status"] == "skipped"))]))
        self.exits.append(self._exits(pre, float(loss), gtd, g1, out))
        action = NONE if pre["frozen"] else ACCEPT if it is not None else TRIAL if out["phase"] in ("bracket", "zoom") else RESTORE
        w = dict(action=action, did=ls_.PHASES.index(out["phase"]), state=ref.state, t=ref.t, slot_new=ref.slot_new, b=tuple(ref.b), bf=tuple(ref.bf),
                 bgtd=tuple(ref.bgtd), bslot=tuple(ref.bslot), low_pos=ref.low_pos, insuf=int(ref.insuf), ls_iter=ref.ls_iter, ls_evals=ref.ls_evals,
                 evals_total=ref.evals_total, accepted=ref.accepted, end_max_ls=ref.end_max_ls, end_width=ref.end_width, end_curv=ref.end_curv,
                 stalled=ref.stalled, frozen=lb.frozen, rec_frozen=float(lb.frozen), f0=ref.f0, gtd0=ref.gtd0, dnorm=ref.dnorm,
                 at_start=int(not lb.frozen and ref.state != ls_.IDLE))
        if action == ACCEPT:
            w.update(t_acc=out["t_acc"], f_acc=it["loss"], from_idle=int(pre["state"] == ls_.IDLE))
            if pre["state"] != ls_.IDLE:
                w.update(lb_t=out["t_acc"])              # s = t_acc d: the step of the pair the iteration forms
            if not froze:
                w.update(gtd_acc=ref.bgtd[1])
        if action == RESTORE:
            w.update(t_acc=pre["t_low"] if pre["state"] == ls_.ZOOM else 0.0, from_idle=0)
        self.want.append(w)
        return out

    def _exits(self, pre, loss, gtd, g1, out):
        """which exits of the machine this tick took, read off the reference's state before and after and its counters"""
        ref, it = self.ref, out["iteration"]
        if pre["frozen"]:
            return {"tick on a frozen state"}
        if pre["state"] == ls_.IDLE:
            e = {"evaluation at theta0"}
        elif out["frozen"] == 2 and it is None:
            e = {"non-finite trial in " + ("zoom" if pre["state"] == ls_.ZOOM else "bracket")}
            return e | ({"non-finite trial in zoom, low end off the start"} if pre["state"] == ls_.ZOOM and pre["t_low"] != 0.0 else set())
        else:
            e = set()
            curv, mx, width, stalled = (a - b for a, b in zip((ref.end_curv, ref.end_max_ls, ref.end_width, ref.stalled), pre["counts"]))
            if pre["state"] == ls_.BRACKET:
                if out["phase"] == "bracket":
                    e.add("extrapolation")
                    if pre["ls_iter"] == 1 and loss >= pre["bf0"]:      # (torch compares with the previous trial from the third on)
                        e.add("extrapolation past a second trial that rose")
                elif curv:
                    e.add("curvature accept in bracket")
                elif pre["ls_iter"] >= ref.max_ls:
                    e.add("max_ls fallback")
                else:                                    # torch's order of tests
                    e.add("bracket by armijo" if loss > pre["f0"] + ref.c1 * pre["t"] * pre["gtd0"] else
                          "bracket by loss >= bf[0]" if pre["ls_iter"] > 1 and loss >= pre["bf0"] else "bracket by gtd >= 0")
            elif curv:
                e.add("curvature accept in zoom")
            if mx:
                e.add("end by max_ls")
            if width:
                e.add("width break")
            if stalled:
                e.add("stalled accept")
            if it is not None and out["t_acc"] != pre["t"]:
                e.add("accepted point is not the last")
            if out["phase"] == "zoom":
                bmax, bmin = max(ref.b), min(ref.b)
                eps = 0.1 * (bmax - bmin)
                for end, at in (("upper", bmax - eps), ("lower", bmin + eps)):
                    if ref.t == at:                      # the flag a ZOOM tick enters with is the one the rule reads (a new bracket clears it)
                        flagged = pre["state"] == ls_.ZOOM and pre["insuf"]
                        e.add(f"insufficient-progress nudge to the {end} end" if flagged else "out-of-bracket nudge")
                if ref.insuf:
                    e.add("insufficient progress flagged")
        if it is not None and it["status"] != "applied":
            e.add("iteration froze" if it["status"] == "frozen" else "iteration skipped")
        return e

    def run(self, fun, n):
        for _ in range(n):
            self.tick(*fun(self.ref.theta))
        return self


def profile(name, phi, dphi, lr, n=60, **kw):
    """a 1-D profile from 0 along d = -phi'(0): ticks until the first search ends, one more"""
    tr = Trace(name, ls_.LbfgsLsRef(np.zeros(1), lr, 3, tolerance_grad=0.0, **kw))
    fun = lambda th: (phi(float(th[0])), np.array([dphi(float(th[0]))]))
    tr.tick(*fun(tr.ref.theta))
    for _ in range(n):
        if tr.tick(*fun(tr.ref.theta))["phase"] in ("accepted", "frozen"):
            break
    tr.tick(*fun(tr.ref.theta))
    return tr


def kinked(a, k):
    """falls with slope -1 up to a, rises with slope k behind it"""
    return (lambda s: -s if s <= a else -a + k * (s - a)), (lambda s: -1.0 if s <= a else k)


def traces():
    T = []
    for problem, (make, P) in PROBLEMS.items():
        for lr in (0.01, 1.0, 8.0):
            for history in (3, 10):
                fun, theta0 = make(P, 7)
                T.append(Trace(f"{problem}_lr{lr}_m{history}", ls_.LbfgsLsRef(theta0, lr, history)).run(fun, 40))
    for case, (make, lr, seed) in cases.TICK_CASES.items():
        for history in (3, 10):
            theta0 = cases.start_params(cases.SHAPE_PARAMS["P1153"])
            obj = make(theta0, seed)
            ref = ls_.LbfgsLsRef(theta0, lr, history, tolerance_grad=1e-30, ring_dtype=np.float32, exact_losses=True)
            T.append(Trace(f"{case}_m{history}", ref).run(lambda th: cases.injected(obj, th), cases.TICKS))
    for name, (phi, dphi, lr, kw, end) in cases.END_CELLS.items():
        kw = dict(kw)
        theta0 = cases.start_params(cases.SHAPE_PARAMS["P1153"])
        obj = cases.LineProfile(theta0, phi, dphi)
        ref = ls_.LbfgsLsRef(theta0, lr, 3, tolerance_grad=1e-30, tolerance_change=kw.pop("tolerance_change", 1e-9), ring_dtype=np.float32,
                             exact_losses=True, **kw)
        tr = Trace("end_" + name, ref).run(lambda th: cases.injected(obj, th), 1)
        for _ in range(70):
            if tr.tick(*cases.injected(obj, ref.theta))["phase"] in ("accepted", "frozen"):
                break
        T.append(tr)
    # the trial after two extrapolations lands behind a kink: below the Armijo line, above the previous trial
    T.append(profile("kink_behind_two_extrapolations", *kinked(5.0, 0.9), lr=0.1))
    # the kink of tests/test_lbfgs_ls_reference_cpu.py on a budget, and the cubic whose minimiser sits just inside an end
    for max_ls in range(2, 12):
        T.append(profile(f"kink_max_ls{max_ls}", lambda s: abs(s - 0.3), lambda s: -1.0 if s < 0.3 else 1.0, lr=1.0, max_ls=max_ls, tolerance_change=1e-12))
    T.append(profile("inside_an_end", lambda s: (s - 0.95) ** 2 + 5.0 * max(0.0, s - 1.0), lambda s: 2 * (s - 0.95) + (5.0 if s > 1.0 else 0.0),
                     lr=1.05, c2=1e-3, max_ls=30, tolerance_change=1e-12))
    # its mirror image: a steep ramp in front of the minimum at 1, the first trial far behind it: the minimiser sits inside the upper end
    T.append(profile("inside_the_upper_end", lambda s: (s - 1.0) ** 2 + 2.0 * max(0.0, 0.7 - s), lambda s: 2 * (s - 1.0) - (2.0 if s < 0.7 else 0.0),
                     lr=2.5, c2=1e-3, max_ls=30, tolerance_change=1e-12))
    # a step up of 0.95 at 0.5 under slope -1: the second trial (t = 1) lies above the first (t = 0.1) and below the Armijo line
    T.append(profile("second_trial_rose", lambda s: -s + (0.95 if s > 0.5 else 0.0), lambda s: -1.0, lr=0.1, max_ls=4))
    # scripted losses: a non-finite trial in zoom and in the bracket phase (then ticks on the frozen state), a loss that rises wherever it
    # is tried (the search closes on t = 0: stalled), a run into tolerance_grad and one under a stop_loss
    fun, theta0 = PROBLEMS["quadratic"][0](8, 3)
    for phase, lr in (("zoom", 8.0), ("bracket", 0.01)):
        tr = Trace("nan_in_" + phase, ls_.LbfgsLsRef(theta0, lr, 3))
        for _ in range(20):
            if tr.tick(*fun(tr.ref.theta))["phase"] == phase:
                break
        tr.tick(float("nan") if phase == "zoom" else 1.0, fun(tr.ref.theta)[1] * (1.0 if phase == "zoom" else float("inf")))
        T.append(tr.run(fun, 2))
    obj, start = PROBLEMS["rosenbrock"][0](16, 7)
    tr = Trace("nan_in_zoom_low_end_moved", ls_.LbfgsLsRef(start, 8.0, 3))
    for _ in range(80):
        tr.tick(*obj(tr.ref.theta))
        if tr.ref.state == ls_.ZOOM and tr.ref.b[tr.ref.low_pos] != 0.0:
            break
    tr.tick(float("nan"), obj(tr.ref.theta)[1])
    T.append(tr.run(obj, 1))
    tr = Trace("rising", ls_.LbfgsLsRef(theta0, 1.0, 3, max_ls=4))
    l0, g0 = fun(theta0)
    tr.tick(l0, g0)
    for k in range(8):
        if tr.tick(l0 + 1.0 + k, g0)["phase"] == "accepted":
            break
    T.append(tr.run(fun, 3))
    T.append(Trace("into_tolerance_grad", ls_.LbfgsLsRef(theta0, 1.0, 10, tolerance_grad=1e-5)).run(fun, 40))
    T.append(Trace("under_stop_loss", ls_.LbfgsLsRef(theta0, 1.0, 10, stop_loss=1e-3)).run(fun, 40))
    T.append(Trace("every_iteration_skipped", ls_.LbfgsLsRef(theta0, 1.0, 3, tolerance_change=1e30)).run(fun, 4))
    return T


@pytest.fixture(scope="module")
def runs():
    return traces()


def test_the_traces_reach_every_exit(runs):
    seen = {}
    for tr in runs:
        for e in tr.exits:
            for x in e:
                seen.setdefault(x, tr.name)
    print("\n".join(f"   {x}: first in {seen.get(x)}" for x in EXITS))
    assert not [x for x in EXITS if x not in seen]
    assert set(seen) <= set(EXITS) | NOT_ASKED


@pytest.fixture(scope="module")
def child(runs, tmp_path_factory):
    """the child's stdout lines, from one sanitizer build and one run over every trace"""
    if shutil.which("g++") is None:
        pytest.fail("no g++ on this host: the rules' sanitizer self-test cannot be built")
    tmp = tmp_path_factory.mktemp("lbfgs_rules")
    exe, trace = str(tmp / "lbfgs_rules_selftest"), str(tmp / "trace.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    with open(trace, "w") as f:
        f.write("\n".join(ln for tr in runs for ln in tr.lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe, trace], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, "sanitizer self-test failed:\n" + out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert got[-1] == f"done {sum(len(tr.want) for tr in runs)}", got[-1]
    return got[:-1]


def _parse(line):
    """NAME K key value [value] ... -> (NAME, K, dict)"""
    t = line.split()
    d, i = {}, 2
    while i < len(t):
        key, n = t[i], 2 if t[i] in ("b", "bf", "bgtd", "bslot") else 1
        vals = [float.fromhex(v) if ("x" in v or v in ("nan", "-nan", "inf", "-inf")) else int(v) for v in t[i + 1:i + 1 + n]]
        d[key] = tuple(vals) if n == 2 else vals[0]
        i += 1 + n
    return t[0], int(t[1]), d


def _bits(v):
    """integers as they are, doubles by their bits (the sign of a zero included; every NaN is one), pairs element by element"""
    if isinstance(v, tuple):
        return tuple(_bits(x) for x in v)
    return int(v) if isinstance(v, (int, np.integer)) else float(v).hex()


def test_the_header_takes_the_reference_s_decisions_bit_for_bit(runs, child):
    lines = iter(child)
    n = 0
    for tr in runs:
        for k, want in enumerate(tr.want):
            name, kk, got = _parse(next(lines))
            assert (name, kk) == (tr.name, k)
            for key, w in want.items():
                assert _bits(got[key]) == _bits(w), (tr.name, k, key, got[key], w, tr.lines[0])
            n += 1
    assert n > 1000
