"""The fp64 sparse-LR oracle of ``_lr_oracle.py`` with one eviction in the
middle, shared by ``test_evict_cpu.py`` (its preconditions, from the oracle
alone) and ``test_gpu_evict.py`` (the engine against it).

``LROracle("adagrad")`` steps over ``O.batches(name, world)``.  After step
index 3 the keys with ``h <= thr`` are removed — ``keys``, ``w``, ``h``, ``dw``
and ``dh`` filtered — and it steps on to 8.  A removed key that reappears is
inserted again from ``init_reference`` with h = 0 and a fresh error budget,
which is what an evicting table must do.

``thr`` is chosen per data set, not hard-coded: the midpoint of the widest gap
between consecutive sorted ``h`` values between the 40th and the 60th
percentile, so that no key's ``h`` sits near the threshold: ``margin`` is
``min |h - thr| / tol_h`` over all keys at that moment (tol_h as
``LROracle.result`` defines it), and a table whose ``h`` is within ``tol_h`` of
the oracle's picks the same victims when ``margin > 1``.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import _lr_oracle as O

EVICT_AFTER = 4  # steps before the eviction (step indices 0..3)


@dataclass
class Evicting:
    res: O.Result        # the final model (keys sorted, w, h, tolerances, losses of all 8 steps)
    thr: float
    n_before: int        # keys when the eviction ran
    evicted: np.ndarray  # the keys removed (sorted)
    margin: float        # min |h - thr| / tol_h at the eviction
    reappear: int        # evicted keys that occur again in steps 4..7


def pick_threshold(h: np.ndarray) -> float:
    hs = np.sort(h)
    n = len(hs)
    lo, hi = int(np.floor(0.4 * n)), int(np.ceil(0.6 * n))
    gaps = hs[lo + 1:hi + 1] - hs[lo:hi]
    i = lo + int(np.argmax(gaps))
    return float(0.5 * (hs[i] + hs[i + 1]))


@functools.lru_cache(maxsize=None)
def evicting_reference(name: str, world: int = 1) -> Evicting:
    orc = O.LROracle("adagrad")
    bs = O.batches(name, world)
    for k, x, y in bs[:EVICT_AFTER]:
        orc.step(k, x, y)
    h = orc.h.astype(np.float64)
    thr = pick_threshold(h)
    tol_h = 1e-7 + 1e-4 * h + orc.dh
    margin = float((np.abs(h - thr) / tol_h).min())
    victim = h <= thr
    evicted = orc.keys[victim].copy()
    n_before = len(orc.keys)
    keep = ~victim
    orc.keys, orc.w, orc.h = orc.keys[keep], orc.w[keep], orc.h[keep]
    orc.dw, orc.dh = orc.dw[keep], orc.dh[keep]
    later = np.unique(np.concatenate([k.reshape(-1) for k, _, _ in bs[EVICT_AFTER:]]))
    reappear = int(np.isin(evicted, later).sum())
    for k, x, y in bs[EVICT_AFTER:]:
        orc.step(k, x, y)
    res = orc.result()
    for a in (res.keys, res.w, res.h, res.tol_w, res.tol_h, evicted):
        a.setflags(write=False)
    return Evicting(res, thr, n_before, evicted, margin, reappear)
