#!/usr/bin/env python
"""tests/golden/create_table.json: what engine creation decides for every cell of tests/create_table.py, recorded from a build of the
commit BEFORE a change to creation (the reference is the parent, never the code under test).  On a GPU machine:

    GPE_HIP_LIB=<libgpe_hip.so built at the parent commit> python tools/create_table.py <parent commit> tests/golden/create_table.json
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpe_pinn import capi               # noqa: E402
from tests import create_table as CT    # noqa: E402


def main(parent, out):
    cells = CT.cells()
    table = {k: CT.record(*cells[k]) for k in sorted(cells)}
    with open(out, "w") as f:
        json.dump({"parent": parent, "cells": table}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} cells from {capi.library_path()} (commit {parent}) -> {out}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
