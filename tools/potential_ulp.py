#!/usr/bin/env python3
"""usage: tools/potential_ulp.py > profiles/potential/values_ulp.txt
U of potential.error_bound on the device: the error of expf / cosf themselves, in ulp, over the inputs of tests/test_gpu_potential_terms.py
(single-term GAUSS and LATTICE tables).  The argument the device hands the function is known bit for bit (t_k and s are correctly rounded
fp32 operations: potential.evaluate(..., float32) restates them), so the reference here is a f(argument_fp32) in fp64 and what remains is the
function's error plus the roundings behind it.  The raw error against the fp64 reference of the whole term is printed too: it carries the
argument's rounding, which error_bound counts separately (the (dim + 3) s and 6 |t_k| parts)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gpe_pinn import potential as pot
from tests import potential_cases as PC
from tests import test_gpu_potential_terms as G          # (its engines, row counts and inputs: the figure is about the test's own inputs)

f = np.float32
out = []
worst = 0.0
for dim, cls in ((1, "coop"), (2, "h128"), (3, "wide")):
    eng = G._engine(G._ctx(cls), None)
    for kind in ("gaussian", "lattice"):
        t = PC.single(kind, dim)[0]
        eng.bind_potential_terms([t])
        m_fn, m_raw = 0.0, 0.0
        for n in G.ROWS:
            x = PC.points(dim, n, seed=n)
            got = eng.potential_at(x).cpu().numpy().astype(np.float64)
            tk = [f(t.w[k]) * (x[:, k] - f(t.c[k])) for k in range(dim)]
            a = float(f(t.a))
            if kind == "gaussian":
                s = np.zeros(n, f)
                for k in range(dim):
                    s = pot._fma32(tk[k], tk[k], s)
                fn = np.exp(-s.astype(np.float64))
                # got = a expf(-s) (1 + d): |err| <= |a| fn eps (2 U + 1)  (expf U ulp <= 2 U eps relative, the product eps)
                U = (np.abs(got - a * fn) / (abs(a) * fn * pot.EPS32) - 1.0) / 2.0
            else:
                on = [k for k in range(dim) if f(t.w[k]) != 0]
                c = [np.cos(tk[k].astype(np.float64)) for k in on]
                fn = sum(ck * ck for ck in c)
                # per axis |d cos^2| <= 2 |c| 2 U eps + eps c^2, the adds and the product with a: |err| <= |a| eps sum_k (2 U + 2) at most
                U = (np.abs(got - a * fn) / (abs(a) * pot.EPS32 * len(on)) - 2.0) / 2.0
            m_fn = max(m_fn, float(U.max()))
            m_raw = max(m_raw, float(PC.ulp_error(got, pot.evaluate([t], x, np.float64)).max()))
        out.append(f"{kind:9s} dim {dim}: function error U = {m_fn:.4f} ulp (raw error of the term against the fp64 reference, argument rounding "
                   f"included: {m_raw:.1f} ulp of V) over rows {G.ROWS}")
        worst = max(worst, m_fn)
    eng.close()
out.append(f"largest: {worst:.4f} ulp -> U_DEVICE = ceil(2 x largest) = {int(np.ceil(2 * max(worst, 0.0)))}")
print("\n".join(out))
