"""Analytic potential terms (include/gpe_hip.h: gpe_potential_terms; csrc/gpe_potential.h): the table an Engine configured with
POT_PRECOMPUTED fills its own V array from -- at every bind and behind every redraw of a sampler -- restated in numpy.

A term is a plain record (kind, a, w, c).  With t_k = w_k (x_k - c_k) for k < dim and s = sum_k t_k^2:
    quadratic  a s          quartic  a s^2          gaussian  a exp(-s)
    lattice    a sum_{k: w_k != 0} cos(t_k)^2       linear    a sum_k t_k
and V(x) = sum_j term_j(x).  evaluate(..., float64) is the reference the device values are held to, within error_bound; evaluate(...,
float32) follows the device's own operation order (fp32 throughout, s by fused multiply-adds in ascending k, the terms added in table
order from 0), which for the terms without exp / cos gives the device's bits.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence

import numpy as np

from . import _capi as capi

QUAD, QUARTIC, GAUSS, LATTICE, LINEAR = 0, 1, 2, 3, 4
KIND_NAMES = ("quadratic", "quartic", "gaussian", "lattice", "linear")
MAX_TERMS = capi.GPE_MAX_POT_TERMS


class Term(NamedTuple):
    kind: int
    a: float
    w: tuple
    c: tuple


def _axes(v, name, fill=0.0):
    v = [float(u) for u in np.atleast_1d(np.asarray(v, dtype=np.float64)).ravel()]
    if not 1 <= len(v) <= 3:
        raise ValueError(f"{name}: 1 to 3 axes")
    return tuple(v + [fill] * (3 - len(v)))


def _term(kind, a, w, c):
    w3 = _axes(w, "w")
    c3 = (0.0, 0.0, 0.0) if c is None else _axes(c, "c")
    return Term(int(kind), float(a), w3, c3)


def quadratic(a, w, c=None) -> Term:
    """a sum_k (w_k (x_k - c_k))^2: an anisotropic harmonic trap about any centre"""
    return _term(QUAD, a, w, c)


def quartic(a, w, c=None) -> Term:
    """a (sum_k (w_k (x_k - c_k))^2)^2: quartic confinement"""
    return _term(QUARTIC, a, w, c)


def gaussian(a, w, c=None) -> Term:
    """a exp(-sum_k (w_k (x_k - c_k))^2): a bump, a dimple or (a < 0) a well; w_k = 1 / (sqrt(2) sigma_k)"""
    return _term(GAUSS, a, w, c)


def lattice(a, w, c=None) -> Term:
    """a sum_{k: w_k != 0} cos(w_k (x_k - c_k))^2: an optical lattice along the axes with w_k != 0"""
    return _term(LATTICE, a, w, c)


def linear(a, w, c=None) -> Term:
    """a sum_k w_k (x_k - c_k): a tilt, gravity"""
    return _term(LINEAR, a, w, c)


def to_c(terms: Sequence[Term]):
    """the ctypes table (gpe_pot_term * n) of a list of terms; what the engine cannot honour it refuses itself"""
    terms = list(terms)
    arr = (capi.gpe_pot_term * max(len(terms), 1))()
    for j, t in enumerate(terms):
        arr[j].kind, arr[j].a = int(t.kind), float(t.a)
        for k in range(3):
            arr[j].w[k], arr[j].c[k] = float(t.w[k]), float(t.c[k])
    return arr


def from_c(arr, n) -> list:
    return [Term(int(arr[j].kind), float(arr[j].a), tuple(float(v) for v in arr[j].w), tuple(float(v) for v in arr[j].c)) for j in range(n)]


def _fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd there (53 bits are
    more than 2 * 24 + 2), and one rounding to float32 follows"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                          # TwoSum: p + c = s + err exactly
    bits = s.view(np.int64).copy()
    inexact = (err != 0.0) & np.isfinite(s)
    toward_zero = inexact & ((err > 0) != (s > 0))           # the exact sum lies between s and its neighbour toward zero: truncate
    bits[toward_zero] -= 1
    bits[inexact] |= 1
    return bits.view(np.float64).astype(np.float32)


def _rows(x):
    x = np.asarray(x)
    if x.ndim != 2 or not 1 <= x.shape[1] <= 3:
        raise ValueError("x must be [N, dim], dim 1 to 3")
    return x


def _parts64(t: Term, x64):
    """(t_k [N, dim], s [N]) of one term in float64, from the float32 values of its constants (what the device holds)"""
    dim = x64.shape[1]
    w = np.array(t.w[:dim], dtype=np.float32).astype(np.float64)
    c = np.array(t.c[:dim], dtype=np.float32).astype(np.float64)
    tk = w * (x64 - c)
    return tk, (tk * tk).sum(axis=1)


def _term64(t: Term, x64):
    tk, s = _parts64(t, x64)
    a = float(np.float32(t.a))
    if t.kind == QUAD:
        return a * s
    if t.kind == QUARTIC:
        return a * s * s
    if t.kind == GAUSS:
        return a * np.exp(-s)
    if t.kind == LATTICE:
        on = np.array([np.float32(v) != 0 for v in t.w[:x64.shape[1]]])
        return a * (np.cos(tk[:, on]) ** 2).sum(axis=1)
    if t.kind == LINEAR:
        return a * tk.sum(axis=1)
    raise ValueError(f"unknown kind {t.kind}")


def evaluate(terms: Sequence[Term], x, dtype=np.float64) -> np.ndarray:
    """V on the points x [N, dim].  float64: the reference (the constants and points rounded to float32 first, as the device holds them,
    everything behind in float64).  float32: the device's operation order in float32."""
    x = _rows(x)
    x32 = x.astype(np.float32)
    if np.dtype(dtype) == np.float64:
        x64 = x32.astype(np.float64)
        V = np.zeros(x.shape[0], dtype=np.float64)
        for t in terms:
            V = V + _term64(t, x64)
        return V
    if np.dtype(dtype) != np.float32:
        raise ValueError("dtype: float64 or float32")
    f = np.float32
    dim = x.shape[1]
    V = np.zeros(x.shape[0], dtype=f)
    for t in terms:
        tk = [f(t.w[k]) * (x32[:, k] - f(t.c[k])) for k in range(dim)]
        s = np.zeros(x.shape[0], dtype=f)
        for k in range(dim):
            s = _fma32(tk[k], tk[k], s)
        a = f(t.a)
        if t.kind == QUAD:
            v = a * s
        elif t.kind == QUARTIC:
            v = a * s * s
        elif t.kind == GAUSS:
            v = a * np.exp(-s)
        elif t.kind == LATTICE:
            l = np.zeros(x.shape[0], dtype=f)
            for k in range(dim):
                if f(t.w[k]) != 0:
                    ck = np.cos(tk[k])
                    l = l + ck * ck
            v = a * l
        elif t.kind == LINEAR:
            l = np.zeros(x.shape[0], dtype=f)
            for k in range(dim):
                l = l + tk[k]
            v = a * l
        else:
            raise ValueError(f"unknown kind {t.kind}")
        V = (V + v).astype(f)
    return V


EPS32 = 2.0 ** -24


def error_bound(terms: Sequence[Term], x, U) -> np.ndarray:
    """Per point, a bound on |V_fp32 - evaluate(terms, x, float64)| by first-order propagation of the fp32 rounding errors, evaluated in
    float64, eps = 2^-24, U the error of expf / cosf in ulp (one ulp of a result is at most 2 eps of its magnitude):

        sum_j |a_j| eps B_j  +  (n_terms - 1) eps sum_j |term_j|

    with s = sum_k t_k^2, t_k = w_k (x_k - c_k), and B_j
        QUAD     (dim + 3) s                    the roundings of t_k carried into t_k^2, the dim fused adds, the product with a
        QUARTIC  (2 dim + 7) s^2                s enters twice, two products
        GAUSS    e^-s (2 U + (dim + 3) s)       |d exp(-s)| = e^-s |ds|; expf itself 2 U eps relative
        LATTICE  sum_{k: w_k != 0} (2 U + 2 + 6 |t_k|)      |d cos^2 t| <= 2 |dt|; cosf 2 U eps on a value <= 1; the square, the add, the product
        LINEAR   3 sum_k |t_k|                  t_k, the adds, the product with a
    The second part is the summation in table order: each of the n_terms - 1 adds rounds a partial sum of magnitude <= sum_j |term_j|.
    These counts are tighter than a strict worst case with every rounding at its extreme and of equal sign (which for an off-centre QUAD
    term is (dim + 5) s: eps each for x_k - c_k and the product with w_k, doubled by the square, dim fused adds, the product with a);
    tests/test_potential_terms_cpu.py prints the largest error / bound it meets (0.93 for a 1D QUAD term, below 0.7 elsewhere)."""
    x = _rows(x)
    x64 = x.astype(np.float32).astype(np.float64)
    dim = x64.shape[1]
    terms = list(terms)
    U = float(U)
    first = np.zeros(x.shape[0])
    mag = np.zeros(x.shape[0])
    for t in terms:
        tk, s = _parts64(t, x64)
        if t.kind == QUAD:
            B = (dim + 3) * s
        elif t.kind == QUARTIC:
            B = (2 * dim + 7) * s * s
        elif t.kind == GAUSS:
            B = np.exp(-s) * (2 * U + (dim + 3) * s)
        elif t.kind == LATTICE:
            on = np.array([np.float32(v) != 0 for v in t.w[:dim]])
            B = (2 * U + 2 + 6 * np.abs(tk[:, on])).sum(axis=1)
        elif t.kind == LINEAR:
            B = 3 * np.abs(tk).sum(axis=1)
        else:
            raise ValueError(f"unknown kind {t.kind}")
        first += abs(float(np.float32(t.a))) * EPS32 * B
        mag += np.abs(_term64(t, x64))
    return first + (len(terms) - 1) * EPS32 * mag
