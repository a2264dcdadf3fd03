"""tests/live_table.py is complete and its rows can fail.

Complete: every entry point of include/gpe_hip.h that changes a live engine -- gpe_set_*, gpe_bind_*, gpe_reset_optimizer,
gpe_keeper_restore, gpe_use_external_exchange, gpe_comm_set_async -- is exercised by a row (its `covers`) or carries a written
exemption.  A new setter fails here until it gets its row, as a new getenv("GPE_...") fails tests/test_switch_table_cpu.py.

Can fail: for every cell whose check is the step-9 record, the fp64 oracle alone tells the problem before the mutation from the one
after it by at least 100 x the loss bound tests/test_gpu_live_engine.py applies (1e-2 relative against 1e-4) -- so an engine that
ignored the mutation, replayed or not, cannot pass.  The start parameters stand in for theta_8, which the CPU cannot know: eight Adam
steps at lr = 1e-3 move each weight by at most about 8e-3."""
import os
import re

import numpy as np
import pytest

from oracle import gpe_oracle as go
from tests import live_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = re.compile(r"^int\s+(gpe_set_\w+|gpe_bind_\w+|gpe_reset_optimizer|gpe_keeper_restore|gpe_use_external_exchange|gpe_comm_set_async)\s*\(", re.M)
FACTOR = 100.0
LOSS_BOUND = 1e-4


def entry_points():
    with open(os.path.join(ROOT, "include", "gpe_hip.h")) as f:
        return set(ENTRY.findall(f.read()))


def covered(rows):
    return {c for r in rows.values() for c in r["covers"]}


def test_every_mutating_entry_point_has_a_row_or_an_exemption():
    names = entry_points()
    assert len(names) >= 20 and {"gpe_set_gamma", "gpe_bind_points", "gpe_keeper_restore"} <= names, sorted(names)      # (the parse itself works)
    have = covered(T.ROWS)
    missing = sorted(names - have - set(T.EXEMPT))
    assert not missing, f"entry points of include/gpe_hip.h with neither a row in tests/live_table.py nor an exemption: {missing}"
    stale = sorted((have | set(T.EXEMPT)) - names)
    assert not stale, f"rows / exemptions for entry points the header no longer declares: {stale}"
    both = sorted(have & set(T.EXEMPT))
    assert not both, f"exempt AND covered by a row: {both}"


def test_the_pattern_catches_a_new_entry_point_and_a_deleted_row():
    src = "int gpe_set_thing(gpe_engine* e, float v);\nint gpe_bind_other (gpe_engine* e);\nint64_t gpe_param_count(const gpe_engine* e);\n" \
          "int gpe_step(gpe_engine* e, gpe_scalars* out);\n/* int gpe_set_hidden(void); */ int gpe_reset_optimizer(gpe_engine* e, float lr);"
    assert set(ENTRY.findall(src)) == {"gpe_set_thing", "gpe_bind_other"}          # (declarations start their line, as the header writes them)
    for name in ("set_gamma", "keeper_restore", "sampler_graded_bound", "bind_base"):
        rows = {k: v for k, v in T.ROWS.items() if k != name}
        assert entry_points() - covered(rows) - set(T.EXEMPT), name              # deleting the row leaves its entry point uncovered


def test_exemptions_carry_reasons_and_name_tests_that_exist():
    assert len(T.EXEMPT) <= 6
    for name, why in T.EXEMPT.items():
        assert len(why.split()) >= 8, name
        for tid in re.findall(r"tests\.\w+::test_\w+", why):
            mod, _, test = tid.partition("::")
            path = os.path.join(ROOT, *mod.split(".")) + ".py"
            assert os.path.exists(path), (name, path)
            with open(path) as f:
                assert re.search(rf"^def {re.escape(test)}\(", f.read(), re.M), (name, tid)


def test_every_row_is_well_formed():
    for name, row in T.ROWS.items():
        assert set(row) == {"group", "classes", "prep", "new", "mutate", "check", "covers", "env", "twin", "note"}, (name, sorted(row))
        assert row["check"] in ("record", "update", "detour") and row["classes"] and set(row["classes"]) <= set(T.CLASSES), name
        assert callable(row["new"]) and callable(row["mutate"]) and row["note"].strip() and "\n" not in row["note"], name
        assert set(row["env"]) <= {"GPE_MERGE_BC", "GPE_GRAPH_STEPS"}, name
        assert row["check"] == "detour" or row["covers"], name
    assert {c for r in T.ROWS.values() for c in r["classes"]} == set(T.CLASSES)
    # rows with bound weights stay at <= 1 024 points (k_head_pde adds with one workgroup: the step is bit-reproducible)
    assert all(c["N"] <= 1024 for c in T.CLASSES.values())


def test_boundary_rows_flip_the_merge_rule_as_they_say():
    for name, want in (("boundary_flips_merge", (True, False)), ("boundary_flips_back", (False, True)), ("boundary_nb_5", (True, True)),
                       ("boundary_nb_own_batch", (False, False)), ("boundary_new_target_own_batch", (False, False))):
        for cls in T.ROWS[name]["classes"]:
            ctx = T.start(cls, T.ROWS[name])
            ctx.setdefault("env", {})
            assert (T.merged(ctx), T.merged(T.ROWS[name]["new"](ctx))) == want, (name, cls)
    ctx = T.start("mix", T.ROWS["points_n_minus_17"])
    assert (T.merged(ctx), T.merged(T.ROWS["points_n_minus_17"]["new"](ctx))) == (True, False)


_START = {}


def _start_loss(name, cls):
    """oracle loss of the start state, shared by the rows of a class that start from the class's plain inputs"""
    row = T.ROWS[name]
    ctx = T.start(cls, row)
    if row["prep"] is not None:
        return ctx, T.oracle(ctx)["loss"]
    if cls not in _START:
        _START[cls] = T.oracle(ctx)["loss"]
    return ctx, _START[cls]


@pytest.mark.parametrize("name,cls", [c for c in T.cells("record") if c[0] != "keeper_restore"], ids=lambda v: v)
def test_the_oracle_tells_the_two_problems_apart(name, cls):
    """|loss_new - loss_old| >= 100 x 1e-4 |loss_new| at the start parameters (for set_params: at the old and the new parameters)"""
    ctx, old = _start_loss(name, cls)
    new = T.oracle(T.ROWS[name]["new"](ctx))["loss"]
    assert np.isfinite(old) and np.isfinite(new)
    assert abs(new - old) >= FACTOR * LOSS_BOUND * abs(new), (name, cls, old, new)


def test_the_kept_and_the_last_parameters_of_the_keeper_row_are_told_apart():
    """keeper_restore puts theta_4 back where theta_8 was.  Neither is known here; the oracle's own fp32 Adam trajectory from the same start
    (lr = 1e-2, as the row sets it) gives both to the round-off of eight steps, and the loss at one differs from the loss at the other
    by far more than 100 x the bound."""
    row = T.ROWS["keeper_restore"]
    ctx = T.start("coop", row)
    assert ctx["env"]["GPE_GRAPH_STEPS"] == "4" and ctx["monitor"]["every"] == 4 and ctx["keeper"]["min_delta"] >= 1e30
    pb = T.problem(ctx)
    st = go.OptState(lr0=ctx["engine_kw"]["lr"])
    th4, _ = go.train_steps(pb, st, ctx["flat"], ctx["x"], 4, ctx["x_bc"])
    th8, _ = go.train_steps(pb, st, th4, ctx["x"], 4, ctx["x_bc"])
    l4, l8 = T.oracle(ctx, th4)["loss"], T.oracle(ctx, th8)["loss"]
    assert abs(l4 - l8) >= FACTOR * LOSS_BOUND * abs(l4), (l4, l8)


def test_update_rows_change_the_optimiser_state_for_real():
    m, v, step = T.adam_state(1000)
    assert step == 5 and np.abs(m).min() > 0 and v.min() > 0 and m.dtype == v.dtype == np.float32
    for name in ("set_lr", "reset_optimizer"):
        for cls in T.ROWS[name]["classes"]:
            assert T.ROWS[name]["new"](T.start(cls))["lr"] >= 2e-3          # twice the lr of the first eight steps (1e-3)
