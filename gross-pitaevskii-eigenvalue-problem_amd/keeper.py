"""The keeper's rule, restated in plain Python (csrc/gpe_observe.h: k_keep_decide, include/gpe_hip.h: gpe_bind_keeper).

The engine judges every monitor record on the device: with m the chosen field (res_rms or energy; lower is better) and best = +inf at
the start, a record improves iff ``isfinite(m) and m < best - min_delta``.  On improvement the record and the parameters are kept and
the count of records since the best returns to 0; otherwise it grows by one, and with ``patience > 0`` the optimiser stops at the first
record where that count reaches ``patience``.  A tie is no improvement, nor is a NaN or an infinity.

`select` applies the same comparisons, in float64 as the kernel does, to a sequence of values -- e.g. one column of
``Engine.read_monitor_array()`` -- so a monitor log can be replayed on the CPU and says which record the engine kept and where it
stopped.  The device goes on judging records after a stop (the parameters are frozen, so their records repeat and improve nothing);
`select` likewise goes through every value it is given.
"""
from __future__ import annotations

import math

METRICS = ("res_rms", "energy")


def select(values, min_delta: float = 0.0, patience: int = 0):
    """-> (kept_index or None, kept_indices, stop_index or None): the index of the record whose parameters are kept at the end, the
    indices of all records that were kept on the way (each an improvement on the one before), and the index of the record at which a
    patience stop fires (None: it never does, always so with patience == 0)."""
    min_delta, patience = float(min_delta), int(patience)
    if not min_delta >= 0.0 or math.isinf(min_delta):
        raise ValueError("min_delta must be finite and >= 0")
    if patience < 0:
        raise ValueError("patience must be >= 0 (0: never stop)")
    best = math.inf
    kept, since, stop = [], 0, None
    for i, v in enumerate(values):
        m = float(v)
        if math.isfinite(m) and m < best - min_delta:
            best, since = m, 0
            kept.append(i)
        else:
            since += 1
        if patience > 0 and since >= patience and stop is None:
            stop = i
    return (kept[-1] if kept else None), kept, stop


def counters(n_values: int, kept_indices):
    """The engine's counters after n_values records, from select's second result: dict(seen, kept, since_best) as
    Engine.keeper_state() reports them."""
    kept_indices = list(kept_indices)
    since = n_values - 1 - kept_indices[-1] if kept_indices else n_values
    return dict(seen=int(n_values), kept=len(kept_indices), since_best=int(since))
