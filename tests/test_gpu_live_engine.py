"""A captured step graph against every setter and rebind of a live engine: the cells of tests/live_table.py.

Protocol of a cell.  Engine A is created under GPE_GRAPH=1, engine B under GPE_GRAPH=0, both from the same start.  GPE_GRAPH=1 forces
gpe_run to replay captured graphs for n_steps >= 8 (GPE_GRAPH_STEPS, default 8), so after run(8) A HOLDS a capture that the mutation
can make stale; B enqueues every step.  On both: run(8), synchronize, theta_8 = get_params(); the row's mutation; run(8), synchronize.

  replay = plain launches, exactly   parameters, both Adam moments and the step counter of A and B equal bit for bit after step 16;
                                     history losses of steps 9 .. 16 to 1e-10 relative (the one atomically summed fp64 term, as
                                     tests/test_gpu_step_state.py grants it)
  the mutation took effect           "record" rows: A's record of step 9 against the fp64 oracle of the MUTATED problem at the parameters
                                     A holds after the mutation -- loss 1e-4, mu 2e-5 relative, the bounds of test_step_matches_oracle
                                     (tests/test_live_table_cpu.py: the old problem is at least 100 x that bound away)
                                     "update" rows (the loss at step 9 cannot move): B runs step 9 by step() and the rest by run(7);
                                     theta_9, m, v against oracle/update_ref.py fed B's state after the mutation and B's own gradient,
                                     element by element within the bounds of tests/test_gpu_update_kernel.py
  "detour" rows                      A makes the call, B does not (an mse_step moves the parameters and is optimiser step 9: B makes it
                                     too, and the eight steps compared are 10 .. 17); same equalities

One engine pair per cell, closed in `finally`; no retries."""
import os

import numpy as np
import pytest

from gpe_pinn import Engine
from tests import live_table as T
from tests.test_gpu_update_kernel import check_elements, ref_for

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _state(eng):
    m, v, step = eng.get_adam_state()
    return eng.get_params(), m, v, step


def _same_state(a, b):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]


def _engine(ctx, graph):
    """an engine in the state ctx describes, created under the row's switches and GPE_GRAPH = graph (set and restored around creation)"""
    env = dict(ctx["env"], GPE_GRAPH=graph)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine(T.config(ctx))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        T.bind_all(eng, ctx)
    except Exception:
        eng.close()
        raise
    return eng


def _check_record(row, ctx, ctx2, A, th8, th):
    first = A.read_history(9, 1)[0]
    assert first["step"] == 9
    if ctx2.get("params") == "set":
        assert np.array_equal(_bits(th), _bits(ctx2["flat"]))
    elif ctx2.get("params") == "kept":
        assert np.array_equal(_bits(th), _bits(A.best_params())) and not np.array_equal(_bits(th), _bits(th8))
        kept, last = T.oracle(ctx2, th)["loss"], T.oracle(ctx2, th8)["loss"]
        print(f"keeper: oracle loss at the kept parameters {kept:.9g}, at theta_8 {last:.9g}")
        assert abs(kept - last) >= 1e-2 * abs(kept), (kept, last)
    else:
        assert np.array_equal(_bits(th), _bits(th8))
    sc = T.oracle(ctx2, th)
    print(f"step 9: loss {first['loss']:.9g} (oracle {sc['loss']:.9g}, rel {abs(first['loss'] - sc['loss']) / abs(sc['loss']):.2e}), "
          f"mu {first['mu']:.9g} (oracle {sc['mu']:.9g}, rel {abs(first['mu'] - sc['mu']) / abs(sc['mu']):.2e})")
    assert abs(first["loss"] - sc["loss"]) <= 1e-4 * abs(sc["loss"]), (first["loss"], sc["loss"])
    assert abs(first["mu"] - sc["mu"]) <= 2e-5 * abs(sc["mu"]), (first["mu"], sc["mu"])


def _step_nine_against_the_update_reference(name, ctx2, B):
    """B's step 9 by step(): the state the mutation left, then theta_9, m, v against the float64 update"""
    th0, m0, v0, step0 = _state(B)
    lr = ctx2.get("lr", B.cfg.lr)
    if ctx2.get("adam") == "zero":
        assert step0 == 0 and not m0.any() and not v0.any()
    elif ctx2.get("adam") == "given":
        gm, gv, gs = T.adam_state(B.n_params)
        assert step0 == gs and np.array_equal(_bits(m0), _bits(gm)) and np.array_equal(_bits(v0), _bits(gv))
    else:
        assert step0 == 8
    ref = ref_for(B, lr=lr)
    ref.theta = th0.astype(np.float64)
    ref.set_adam_state(m0, v0, step0)
    rec = B.step()
    r = ref.update(B.get_grad(), rec["loss"])
    assert r["status"] == "applied" and rec["step"] == step0 + 1 == ref.step
    assert abs(rec["lr"] - r["lr"]) <= 1e-12 * r["lr"] and rec["lr"] == float(np.float32(lr)), (rec["lr"], r["lr"], lr)
    check_elements(_state(B), r, m0.astype(np.float64), name)


@pytest.mark.parametrize("name,cls", T.cells(), ids=lambda v: v)
def test_cell(name, cls):
    row = T.ROWS[name]
    ctx = T.start(cls, row)
    ctx2 = row["new"](ctx)
    A = B = None
    try:
        A, B = _engine(ctx, "1"), _engine(ctx, "0")
        for e in (A, B):
            e.run(8)
            e.synchronize()
        th8 = A.get_params()
        assert _same_state(_state(A), _state(B)) and _state(A)[3] == 8
        row["mutate"](A, ctx2)
        if row["check"] != "detour" or row["twin"]:
            row["mutate"](B, ctx2)
        th = A.get_params()
        A.run(8)
        if row["check"] == "update":
            _step_nine_against_the_update_reference(f"{name}-{cls}", ctx2, B)
            B.run(7)
        else:
            B.run(8)
        A.synchronize(); B.synchronize()
        if row["check"] == "record":                  # first, so that a stale replay is reported as what it is: the old problem's loss
            _check_record(row, ctx, ctx2, A, th8, th)
        elif row["check"] == "detour" and not row["twin"]:
            assert np.array_equal(_bits(th), _bits(th8))
        sa, sb = _state(A), _state(B)
        first = 1 if ctx2.get("adam") == "zero" else (6 if ctx2.get("adam") == "given" else 9)      # (the step counter a reset / restore leaves)
        if row["twin"]:
            first += 1                                                  # (the detour was an Adam step of its own: mse_step took number 9)
        assert sa[3] == sb[3] == first + 7, (sa[3], sb[3])
        assert _same_state(sa, sb), [int((_bits(p) != _bits(q)).sum()) for p, q in zip(sa[:3], sb[:3])]
        la = np.array([h["loss"] for h in A.read_history(first, 8)])
        lb = np.array([h["loss"] for h in B.read_history(first, 8)])
        assert np.all(np.isfinite(lb)) and np.all(np.abs(la - lb) <= 1e-10 * np.abs(lb)), (la, lb)
    finally:
        for e in (A, B):
            if e is not None:
                e.close()
