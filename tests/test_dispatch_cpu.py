"""The pickers of csrc/gpe_dispatch.h (runtime values to template arguments: pick_int, pick_n_out, pick_ce and their each_* twins) under
the address and undefined-behaviour sanitizers.  tests/dispatch_selftest.cpp includes that header alone; it is built here with
g++ -fsanitize=address,undefined and run as a child process -- no GPU, nothing loaded into Python -- once as the product compiles the
header and once with -DGPE_FAST_BUILD.  For every range the launchers use and every input from Lo - 2 to Hi + 2: the lambda is called
exactly once, with the clamped value; the (C, E) pickers accept exactly the pairs the header's comment lists."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dispatch_selftest.cpp")

FULL = ["range 1..5 ok", "range 1..3 ok", "range 0..1 ok", "range 0..3 ok", "range 1..2 ok", "ce_train ok: 4 pairs", "ce_forward ok: 6 pairs",
        "ce_h128_forward ok: 4 pairs", "ce_h128_reverse ok: 3 pairs", "n_out 1..2 ok", "done 0"]
FAST = FULL[:5] + ["ce_train ok: 3 pairs", "ce_forward ok: 3 pairs"] + FULL[7:9] + ["n_out 1..1 ok", "done 0"]


@pytest.mark.parametrize("flags,want", [((), FULL), (("-DGPE_FAST_BUILD",), FAST)], ids=["full", "fast"])
def test_pickers_under_the_sanitizers(tmp_path, flags, want):
    if shutil.which("g++") is None:
        pytest.fail("no g++ on this host: the dispatch self-test cannot be built")
    exe = str(tmp_path / "dispatch_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Werror", *flags, "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, "dispatch self-test failed:\n" + out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.splitlines() == want
