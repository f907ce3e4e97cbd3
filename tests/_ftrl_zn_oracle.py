"""FTRL-Proximal in compact ``[z | n]`` rows (``ftrl_zn``) in fp64 with an
error bound, planted rows and planted mutants.

The maths uses nothing of the project: the pulled weight and the step are
written over ``_opt_oracle.N`` (a value with a running error bound), the step
through ``_opt_oracle.ftrl`` itself.

    w(z, n) = +0                                            if |z| <= l1
              -(z - sign(z) l1) / ((beta + sqrt(n)) / alpha + l2)   otherwise
    step    w = w(z, n) ;  n' = n + g^2 ;  sigma = (sqrt(n') - sqrt(n)) / alpha
            z' = z + (g - sigma w)          (g after grad_scale and clip)

A row stores (z', n') and no w.  From a zero row this is the trajectory of
``_opt_oracle.ftrl`` (w materialised) in exact arithmetic: there the stored w
is w(z, n) of the row's own (z, n) after every step.

The bound is ``_opt_oracle``'s: every operation adds one rounding to the
first-order propagation of its operands' bounds, times ``SAFETY = 2``; the
weight's bound goes into the step (``step`` hands ``ftrl`` the ``N`` that
``weight`` returned).  A correct fp32 evaluation stays within half of it
(``test_ftrl_zn_cpu.py``).

Planted rows (``planted``): the (z, n) pairs of ``_opt_oracle.planted_states``
for FTRL crossed with ``planted_grads``, and threshold rows with ``|z| <= l1``
on input — w = 0 there, so z' = z + g' exactly (g' the scaled gradient,
checked in fp64): they land z' exactly on +-l1 and one fp32 ulp to either side.

Mutants (``MUTANTS``), each outside the bound on a planted coordinate:
    zn_pull_is_z    the pull returns z
    zn_no_sigma_w   the update uses w = 0
    zn_w_no_beta    the pulled w leaves out beta
    zn_neg_zero     -0.0 where w = 0 (``ratio`` with ``ftrl_w``: a zero of the
                    wrong sign is outside)
"""
from __future__ import annotations

import numpy as np

import _opt_oracle as O
from _opt_oracle import N, as_n

MUTANTS = ("zn_pull_is_z", "zn_no_sigma_w", "zn_w_no_beta", "zn_neg_zero")
L1 = 0.3   # the third rule setting beside ("ftrl", "plain") and ("ftrl", "reg")


def settings() -> dict:
    """The rule settings the tests use: name -> ``Hyper`` (fp32 numbers)."""
    return {"plain": O.setting("ftrl", "plain"), "reg": O.setting("ftrl", "reg"),
            "l1": O.Hyper("ftrl", l1=L1).f32()}


def weight(h: O.Hyper, z: N, n: N, mutant=None) -> N:
    """The pulled value w(z, n)."""
    if mutant == "zn_pull_is_z":
        return z
    T, l1 = z.T, z.T(h.l1)
    inside = np.abs(z.v) <= l1
    # the shrink: a 1-Lipschitz selection and one subtraction
    shr = N._rnd(np.where(inside, T(0), z.v - np.sign(z.v) * l1), z.e)
    r = n.sqrt()
    den = (r if mutant == "zn_w_no_beta" else r + h.ftrl_beta) / h.ftrl_alpha + h.l2
    with np.errstate(divide="ignore", invalid="ignore"):
        q = -(shr / den)
    zero = T(-0.0) if mutant == "zn_neg_zero" else T(0)
    return N(np.where(inside, zero, q.v), q.e)


def step(h: O.Hyper, z, n, g, T=np.float64, mutant=None, track=True):
    """One step on every coordinate: ``(z', n')`` as ``N``.  Inputs: arrays
    (exact) or ``N`` (a running bound goes on)."""
    z, n, g = as_n(z, T, track), as_n(n, T, track), as_n(g, T, track)
    if mutant == "zn_no_sigma_w":
        w = N(np.zeros_like(z.v), None if z.e is None else 0.0)
    else:
        w = weight(h, z, n, mutant)
    _, z2, n2 = O.ftrl(h, w, z, n, g)
    return z2, n2


def pull_ratio(h: O.Hyper, rows: np.ndarray, got: np.ndarray):
    """(|got - w(z, n)| / bound per row, the oracle's w) for fp32 rows
    [m, 2]; a zero of the wrong sign where w = 0 is outside."""
    ref = weight(h, as_n(rows[:, 0]), as_n(rows[:, 1]))
    return O.ratio(ref, np.asarray(got).reshape(-1), ftrl_w=True), ref


def rows_ratio(parts, got: np.ndarray) -> np.ndarray:
    """``ratio`` of rows ``got`` [m, 2] against ``step``'s (z', n')."""
    return np.stack([O.ratio(parts[0], got[:, 0]), O.ratio(parts[1], got[:, 1])], axis=1)


# ---------------------------------------------------------- planted inputs
def planted_threshold(h: O.Hyper):
    """(z, n, g) with |z| <= l1 on input (w = 0, so z' = z + g' exactly) whose
    z' lands exactly on +-l1 and one fp32 ulp of z to either side."""
    s, l1 = np.float32(h.grad_scale), np.float32(h.l1)
    g = np.float32(0.0625)
    ge = np.float64(g) * np.float64(s)
    assert h.clip == 0 or ge < h.clip
    z0 = np.float32(np.float64(l1) - ge)
    assert np.float64(z0) + ge == np.float64(l1), "planted threshold is not exact"
    up, dn = np.nextafter(z0, np.float32(np.inf)), np.nextafter(z0, np.float32(-np.inf))
    out = []
    for sign in (1.0, -1.0):
        for z in (z0, up, dn):
            if abs(np.float64(z)) > np.float64(l1):   # l1 = 0: only z = 0 is inside
                continue
            for n in (0.0, 0.5):
                out.append((sign * z, n, sign * g))
    if l1 == 0:   # z' = g' exactly, from z = +-0
        out += [(0.0, 0.0, g), (0.0, 0.5, -g), (-0.0, 0.5, g)]
    a = np.asarray(out, np.float32)
    assert (np.abs(a[:, 0]) <= l1).all()
    return a[:, 0], a[:, 1], a[:, 2]


def planted(h: O.Hyper):
    """Every planted (z, n) crossed with every planted gradient, then the
    threshold rows: flat fp32 arrays (z, n, g)."""
    g = O.planted_grads(h)
    _, z, n = O.planted_states(h)
    Z, Nn, G = np.repeat(z, len(g)), np.repeat(n, len(g)), np.tile(g, len(z))
    tz, tn, tg = planted_threshold(h)
    return np.concatenate([Z, tz]), np.concatenate([Nn, tn]), np.concatenate([G, tg])


def gaussian(h: O.Hyper, m: int, seed: int = 0):
    """Seeded ordinary coordinates (z, n, g)."""
    _, z, n, g = O.gaussian(h, m, seed)
    return z, n, g


def table_rows(h: O.Hyper, nkeys: int, seed: int = 0) -> np.ndarray:
    """Initial rows [nkeys, 2]: the planted (z, n) first (aligned with
    ``table_grads(step 0)``), seeded ordinary states on the rest."""
    pz, pn, _ = planted(h)
    gz, gn, _ = gaussian(h, nkeys, seed)
    k = min(len(pz), nkeys)
    gz, gn = gz.copy(), gn.copy()
    gz[:k], gn[:k] = pz[:k], pn[:k]
    return np.stack([gz, gn], axis=1).astype(np.float32)


def table_grads(h: O.Hyper, nkeys: int, step_no: int, seed: int = 0) -> np.ndarray:
    """Gradients [nkeys, 1] of step ``step_no``: even steps the planted
    gradients (aligned with ``table_rows`` at step 0, rolled by the step
    after), odd steps seeded Gaussian."""
    if step_no % 2:
        return np.random.default_rng(1000 + 17 * seed + step_no).standard_normal(
            (nkeys, 1)).astype(np.float32)
    return O.fill(planted(h)[2], (nkeys, 1), roll=0 if step_no == 0 else 7 * step_no + 1)
