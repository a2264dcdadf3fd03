"""The switch table (tests/switch_table.py) names every GPE_* variable the library reads, and nothing else: a new read in the
sources fails here until its row -- values, the classes it applies to, what the switch matrix expects of it -- is added.  A read is a
call of one of csrc/gpe_env.h's readers (or a raw getenv) with the switch's name as a string literal."""
import os
import re

from tests import switch_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gross-pitaevskii-eigenvalue-problem_amd", "csrc")
UNITS = ("gpe_engine.hip", "gpe_wide.hip")

READERS = ("env_set", "env_on", "env_opt_in", "env_int", "env_i64", "env_int_in", "env_i64_in")
GETENV = re.compile(r'\b(?:getenv|' + "|".join(READERS) + r')\(\s*"(GPE_[A-Z0-9_]+)"\s*[,)]')
ANY_READ = re.compile(r'\b(?:getenv|' + "|".join(READERS) + r')\s*\(')


def switches_read():
    names = set()
    for u in UNITS:
        with open(os.path.join(CSRC, u)) as f:
            names |= set(GETENV.findall(f.read()))
    return names


def test_the_units_read_the_switches_the_table_names():
    read = switches_read()
    assert len(read) >= 40, sorted(read)                 # (the parse itself works)
    missing = sorted(read - set(T.SWITCHES))
    stale = sorted(set(T.SWITCHES) - read)
    assert not missing, f"switches read by the library without a row in tests/switch_table.py: {missing}"
    assert not stale, f"rows in tests/switch_table.py for switches the library no longer reads: {stale}"


def test_getenv_pattern_catches_a_new_switch():
    src = 'int x; { const char* v = getenv("GPE_NEW_THING"); }  getenv( "GPE_OTHER" )'
    assert set(GETENV.findall(src)) == {"GPE_NEW_THING", "GPE_OTHER"}
    for i, r in enumerate(READERS):
        for call in (f'e->x = {r}("GPE_NEW_{i}");', f'if ({r}( "GPE_NEW_{i}" , e->x, 1, 2)) y();', f'{r}("GPE_NEW_{i}",0)'):
            assert GETENV.findall(call) == [f"GPE_NEW_{i}"], call
    assert not GETENV.findall('my_env_on("GPE_X"); env_on(name); env_int("OTHER_X", 0)')


def test_no_read_hides_behind_a_name_that_is_no_literal():
    """every getenv / reader call of the two units is one the pattern catches; gpe_env.h alone calls getenv with a variable"""
    with open(os.path.join(CSRC, "gpe_env.h")) as f:
        assert set(re.findall(r"static inline \w+ (\w+)\(", f.read())) == set(READERS)      # (READERS names every reader there is)
    for u in UNITS:
        with open(os.path.join(CSRC, u)) as f:
            src = f.read()
        assert len(ANY_READ.findall(src)) == len(GETENV.findall(src)), \
            f"{u}: a getenv / env_* call whose argument is not a \"GPE_...\" literal: " \
            + str([ln.strip() for ln in src.split("\n") if ANY_READ.search(ln) and len(ANY_READ.findall(ln)) != len(GETENV.findall(ln))])
    assert ANY_READ.search('x = getenv (name);') and ANY_READ.search("env_int(n, 0)") and not ANY_READ.search("my_getenv(name)")


def _descriptor(**kw):
    d = dict(H=64, maps=3, res=False, n_out=1, dim=2, path="fused", loss="plain", pad=False, large=False, P=12801)
    d.update(kw)
    assert set(d) == set(T.CLASS_KEYS)
    return d


def test_every_row_is_well_formed():
    probes = [_descriptor(), _descriptor(H=32, dim=1, maps=2), _descriptor(res=True, maps=2), _descriptor(H=128, path="wide", P=66000),
              _descriptor(path="generic", H=64), _descriptor(large=True), _descriptor(pad=True), _descriptor(n_out=2, loss="plain"),
              _descriptor(H=256, dim=3, path="wide", P=140000)]
    for name, row in T.SWITCHES.items():
        assert set(row) <= {"values", "applies_to", "expect", "note", "multi", "dp"}, (name, sorted(row))
        exp = row["expect"]
        assert exp in T.EXPECTS or exp.startswith("elsewhere:"), (name, exp)
        assert row["values"], name
        for v in row["values"]:
            assert isinstance(v, dict) and name in v, (name, v)          # every value sets its own switch
            assert all(k.startswith("GPE_") and isinstance(s, str) for k, s in v.items()), (name, v)
        assert row["note"].strip() and "\n" not in row["note"], name
        assert callable(row["applies_to"])
        hits = [bool(row["applies_to"](d)) for d in probes]
        assert any(hits), f"{name}: applies to none of the probe classes"


def test_elsewhere_rows_name_tests_that_exist():
    for name, row in T.SWITCHES.items():
        if not row["expect"].startswith("elsewhere:"):
            continue
        tid = row["expect"][len("elsewhere:"):]
        mod, _, test = tid.partition("::")
        assert mod.startswith("tests.") and test.startswith("test_"), (name, tid)
        path = os.path.join(ROOT, *mod.split(".")) + ".py"
        assert os.path.exists(path), (name, path)
        with open(path) as f:
            assert re.search(rf"^def {re.escape(test)}\(", f.read(), re.M), (name, tid)
