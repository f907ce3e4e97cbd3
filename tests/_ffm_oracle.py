"""A high-precision field-aware FM reference with a derived error bound, its
data sets and its planted mutants.  Built like ``_fm_oracle.py``; shares
``_lr_oracle.Dataset`` (and its libsvm writer), ``EMPTY``, ``U32``, ``U_G``,
``_fm_oracle.U_A`` and ``_lr_oracle.update`` (``_opt_oracle``'s rules).

The model (``FFMOracle``), rows ``[w | v_0 .. v_{F-1}]``, dim = 1 + F K
---------------------------------------------------------------------
The one of the ``models/ffm.py`` docstring, in fp64 on ``[B, F]`` key arrays.
Every non-EMPTY occurrence (s, i) is a feature of field i (its column).  With
``R_i`` the row of occurrence i and ``R_i[j]`` its block j:

    z_s = sum_i w_i + sum_{i<j} <R_i[j], R_j[i]>      g_s = sigmoid(z_s) - y_s
    per occurrence:  dw = g_s,  dR_i[j] = g_s R_j[i] (j != i, j an occurrence)

A key at two columns i, j of a sample is two occurrences with the cross term
``<R[j], R[i]>`` of the one row.  Gradients are summed per distinct key over
the batch (the union batch at world 2), then one SGD / AdaGrad update per key
and step.  The diagonal block ``R_i[i]`` and untouched keys do not move.

The bound
---------
u = 2^-24.  The kernel forms z as an ordered-pair sum, ``sum_{c=0} a + 1/2
sum_{j != i} a b`` (the halving is exact), over n = F dim elements: a lane adds
a chain of L = ceil(n / G) terms (one FMA each: one rounding, charged two),
``group_sum`` adds log2(min(G, 64)) levels and G = 256 adds the four ``sred``
partials (3 more).  With A_s = sum_i |w_i| + sum_{i<j} sum_k |R_i[j]_k
R_j[i]_k| (the ordered magnitudes, halved):

    dz_s = (L + 1 + log2(min(G, 64)) + 3 [G = 256]) u A_s          (``depth``)

g_s is known to ``r_s = |g_s| (U_G + (1 - |g_s|) dz_s) + U_A`` (``_lr_oracle``
and ``_fm_oracle`` derive U_G and U_A), and for a key with n occurrences and
partner values b (1 for w):

    eG = sum_occ [ r_s |b| + u |g_s b| ] + n u sum_occ |g_s b|

(each product's rounding; n float atomics in any order).  The parameter and
state steps take eG through ``_opt_oracle``'s propagation (``N``), which adds
the update's own roundings (AdaGrad's reciprocal square root at 1 ulp); the
tolerance is ``SAFETY = 2`` times that, so a correct fp32 evaluation stays
within half.  There is no ``1e-6 + 1e-4 |x|`` term.  A key-step is
*ill-conditioned* where ``eG > 0.1 sqrt(h_after + eps)`` (AdaGrad) or the
propagated bound is not finite; there the step is bounded monotonically in G
(``x(G - eG)``, ``x(G + eG)``; the AdaGrad step is monotone in G) plus the
roundings of the step at G.  ``ill`` counts them: 0 on every data set at world
1 and 2, asserted.  No key is excused and no coordinate is widened.

``pred``: ``p (1 - p) (dz + 2 u |z|) + min(p, 1 - p) U_G + U_A`` (2 u |z|: the
two roundings of ``__expf``'s argument).  The loss of a sample: ``|g| dz`` (its
derivative is g) + ``e / (1 + e) (U_G + 2 u |z|)`` + 4 u (the logarithm: 1 ulp
of log2 and the constant, on a value below ln 2; the rounding of 1 + e) + 2 u
(|max(z, 0)| + |y z| + loss) (the two additions).  The batch's sum adds
``(9 + ceil(blocks / 256) + 16) u sum loss``: ``block_sum_256`` (six shuffle
levels, three additions), the atomics into a shard of the counter, and the
fp32 sum of the 256 shards' words.  Both times SAFETY.

SGD has no denominator: ``free_running`` carries the bound from step to step,
through the update (``N``) and, to first order, through the forward: a row
known to dx moves a partner by dx, z by ``sum |a| dx_b``, hence
``eG += sum_occ (|g| dx_b + |b| / 4 * dz_carry)``.

Data sets (``dataset(name)``; 8 steps; libsvm text; seeded)
-----------------------------------------------------------
``ffm_mid`` (F 13, K 4, B 512), ``ffm_wide`` (F 39, K 4, B 512), ``ffm_small``
(F 5, K 2, B 500: the last workgroup has 4 live groups of 16).  Rows hold
3..F entries at random columns, the rest EMPTY; the text writes the EMPTY key
itself into the gaps before a row's last entry, so the field of an occurrence
is its column and not its rank.  Per batch: sample 0 all EMPTY, sample 1 a
single entry, samples 2..11 one key at two columns, keys with exactly 1, 2,
63, 64 and 65 occurrences, and ``HOT`` in ``N_HOT[name][0]`` samples at column
``HOT_COLS[0]`` and in 50 more at ``HOT_COLS[1]``.  A quarter of the drawn keys
carry bits at or above 2^32.  Labels: Bernoulli draws of a planted linear
model.  Initial rows: normal, scale ``INIT_SCALE[name]`` ~ (F (F - 1) K /
2)^-1/4 (the pair part of z at step 0 has a standard deviation of 0.5..1.5),
AdaGrad state ``STATE_INIT`` = 0.01.  With a state of 0 a coordinate's first
step divides by |G| itself, and among the keys with 13..350 occurrences a
few coordinates per batch have a |G| that cancels to below ten times its eG
(``ffm_wide``: 7 key-steps, all at step 0, eG 1e-5..5e-4 from dz): the rule for
ill-conditioned key-steps finds them whatever the seed.  The planted state
keeps the denominator at 0.1 and above.  The first step from a state of 0 is
held too: a case per data set starts from state 0 and asserts the count of
ill-conditioned key-steps (``ILL_FROM_STATE_0``), which the monotone bound
holds (fp32 floor there: x 0.37-0.44, h 0.42-0.46).

Measured on the CPU (``test_ffm_oracle_cpu.py`` prints them as ``CALIBRATION``)
-----------------------------------------------------------------------------
fp32 emulation of the kernel's arithmetic (ordered pairs, lane chains and
shuffle trees on permuted elements, permuted atomics), three permutations,
step by step, largest |fp32 - fp64| / tolerance (x, h, summed loss):

    ffm_mid    adagrad  x 0.477  h 0.490  loss 0.001    sgd  x 0.498  loss 0.001
    ffm_wide   adagrad  x 0.488  h 0.494  loss 0.000    sgd  x 0.497  loss 0.000
    ffm_small  adagrad  x 0.460  h 0.462  loss 0.001    sgd  x 0.497  loss 0.001

Free-running SGD on ``ffm_mid`` against the carried bound: 0.497.  These sit
just under 0.5 for the reason ``_opt_oracle.py`` gives: on a coordinate whose
gradient is exact or 0 the bound is twice the update's own roundings, and one
rounding of a result just above a power of two is half of that by itself; the
gradient's part (eG) is a worst case and is nowhere near attained.  The pair
part of z at step 0 has a standard deviation of 0.71 / 0.73 / 0.93, max |z|
over 8 steps is 4.5 / 5.8 / 7.4 (mid / wide / small), no key-step is
ill-conditioned at world 1 or 2.

Mutants, two steps each, step by step; the smallest max ratio over the three
data sets (x with both rules, h with AdaGrad, the summed loss where the mutant
is wrong in z):

    pair_twice             x 3.1e4   h 2.2e6   loss 4.4e3
    diag_included          x 5.1e4   h 3.7e8   loss 2.0e3
    same_block             x 3.1e6   h 2.9e8   loss 1.7e3
    field_by_rank          x 5.0e6   h 5.2e8   loss 5.3e2
    empty_as_id0           x 7.3e6   h 2.8e8   loss 2.7e2
    dup_once               x 8.7e4   h 4.8e5
    dup_no_self_pair       x 4.5e4   h 3.7e5   loss 9.6
    w_once_per_key         x 8.7e4   h 3.1e6
    drop_65th              x 1.4e3   h 7.6e3
    update_per_occurrence  x 1.2e5   h 7.9e6   (AdaGrad; under SGD, which is
                           linear in G, it is the same function and no mutant)
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import _opt_oracle as _opt
from _fm_oracle import U_A
from _lr_oracle import EMPTY, U32, U_G, Dataset, update

STEPS, EPS = 8, 1e-8
SAFETY = _opt.SAFETY
F = {"ffm_mid": 13, "ffm_wide": 39, "ffm_small": 5}
K = {"ffm_mid": 4, "ffm_wide": 4, "ffm_small": 2}
BATCH = {"ffm_mid": 512, "ffm_wide": 512, "ffm_small": 500}
INIT_SCALE = {"ffm_mid": 0.25, "ffm_wide": 0.15, "ffm_small": 0.55}
STATE_INIT = 0.01   # AdaGrad state of a new key (module docstring)
LR = {"adagrad": 0.05, "sgd": 1e-3}
SEEDS = {"ffm_mid": 21, "ffm_wide": 22, "ffm_small": 23}
N_HOT = {"ffm_mid": (400, 50), "ffm_wide": (300, 50), "ffm_small": (400, 50)}
HOT_COLS = (1, 3)
HOT = np.uint64(2_100_001)
COUNTS = (1, 2, 63, 64, 65)
PLANTED = {c: np.uint64(2_100_100 + c) for c in COUNTS}
MANDELBROT_Q, RANKS = 50.0, 200_000
MUTANTS = ("pair_twice", "diag_included", "same_block", "field_by_rank", "empty_as_id0",
           "dup_once", "dup_no_self_pair", "w_once_per_key", "drop_65th", "update_per_occurrence")


def geometry(nf: int, k: int):
    """(dim, lanes per sample G, rows a walk step advances di) of the kernel."""
    dim = 1 + nf * k
    G = 16 if nf * dim <= 128 else (64 if nf <= 16 else 256)
    return dim, G, G // dim


def depth(nf: int, k: int) -> int:
    """Roundings on the longest path of the kernel's z sum (module docstring)."""
    dim, G, _ = geometry(nf, k)
    return -(-nf * dim // G) + 1 + int(np.log2(min(G, 64))) + (3 if G == 256 else 0)


# ------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def dataset(name: str) -> Dataset:
    rng = np.random.default_rng(SEEDS[name])
    nf, B = F[name], BATCH[name]
    rows = B * STEPS
    n = rng.integers(3, nf + 1, rows)
    mask = np.argsort(np.argsort(rng.random((rows, nf)), axis=1), axis=1) < n[:, None]
    x = MANDELBROT_Q * ((1.0 + RANKS / MANDELBROT_Q) ** rng.random((rows, nf)) - 1.0)
    r = np.minimum(x.astype(np.int64) + 1, RANKS)
    idx = (r * 7919 % 2_000_003 + 1).astype(np.uint64)
    idx = np.where(idx % np.uint64(4) == 0,  # a quarter of the indices above 2^32
                   idx | ((idx % np.uint64(7) + np.uint64(1)) << np.uint64(32)), idx)
    c1, c2 = HOT_COLS
    for t in range(STEPS):
        b = np.arange(t * B, (t + 1) * B)
        mask[b[0]] = False                                   # all EMPTY
        mask[b[1]] = np.arange(nf) == rng.integers(nf)       # a single entry
        for s in b[2:12]:                                    # one key at two columns
            i, j = np.nonzero(mask[s])[0][[0, -1]]
            idx[s, j] = idx[s, i]
        free = rng.permutation(b[12:])
        h1, h2 = N_HOT[name]
        mask[free[:h1], c1] = True
        idx[free[:h1], c1] = HOT
        mask[free[h1:h1 + h2], c2] = True
        idx[free[h1:h1 + h2], c2] = HOT
        hot = np.zeros((B, nf), bool)
        hot[free[:h1] - b[0], c1] = hot[free[h1:h1 + h2] - b[0], c2] = True
        for c in COUNTS:  # exactly c occurrences, in c different samples
            left = c
            for s in rng.permutation(b[12:]):
                ok = np.nonzero(mask[s] & ~hot[s - b[0]] & ~np.isin(idx[s], list(PLANTED.values())))[0]
                if left and len(ok):
                    idx[s, rng.choice(ok)] = PLANTED[c]
                    left -= 1
    keys = np.where(mask, idx, EMPTY)
    # labels from a planted linear model over the distinct keys (planted keys neutral)
    u, inv = np.unique(keys, return_inverse=True)
    truth = rng.normal(0.0, 1.0, len(u))
    truth[np.isin(u, [HOT, EMPTY] + list(PLANTED.values()))] = 0.0
    z = (truth[inv.reshape(rows, nf)] * mask).sum(1) - 0.5
    y = (rng.random(rows) < 1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    lines = []
    for i in range(rows):  # the EMPTY key itself fills the gaps before the last entry
        last = np.nonzero(mask[i])[0]
        ent = [str(int(k)) for k in keys[i, :last[-1] + 1]] if len(last) else []
        lines.append((" ".join([str(int(y[i]))] + ent) + "\n").encode())
    return Dataset(name, keys, mask.astype(np.float32), y, lines)


def batches(name: str, world: int = 1, steps: int = STEPS):
    """Per step the union batch (keys, y) of ``world`` ranks (B / world rows
    each, concatenated in rank order): a synchronous round's batch."""
    ds, B = dataset(name), BATCH[name]
    out = []
    for t in range(steps):
        parts = [ds.batch(t, B // world, r, world) for r in range(world)]
        out.append(tuple(np.concatenate([p[i] for p in parts]) for i in (0, 2)))
    return out


# ------------------------------------------------------------------ model
def _occ_rank(inv: np.ndarray):
    """Number of each occurrence within its key's list (in occurrence order)."""
    order = np.argsort(inv, kind="stable")
    k = inv[order]
    rank = np.empty(len(inv), np.int64)
    rank[order] = np.arange(len(k)) - np.searchsorted(k, k)
    return rank


def _kernel_sum(terms: np.ndarray, G: int, rng) -> np.ndarray:
    """fp32 sum of ``terms`` [B, n] as the kernel forms it: elements dealt to
    G lanes (in a permuted order), a sequential chain per lane, a shuffle
    tree over up to 64 lanes, and the four partials of G = 256 in order."""
    nb, n = terms.shape
    L = -(-n // G)
    t = np.zeros((nb, L * G), np.float32)
    t[:, :n] = terms[:, rng.permutation(n)]
    t = t.reshape(nb, L, G)
    acc = np.zeros((nb, G), np.float32)
    for l in range(L):
        acc = acc + t[:, l]
    acc = acc.reshape(nb, -1, min(G, 64))
    while acc.shape[2] > 1:
        h = acc.shape[2] // 2
        acc = acc[:, :, :h] + acc[:, :, h:]
    out = acc[:, 0, 0]
    for q in range(1, acc.shape[1]):
        out = out + acc[:, q, 0]
    return out


@dataclass
class Grad:
    u: np.ndarray       # distinct keys of the batch, sorted
    G: np.ndarray       # [nu, D] summed gradient (dtype of the model)
    eG: np.ndarray      # [nu, D] its bound (fp64)
    z: np.ndarray
    p: np.ndarray
    loss: np.ndarray    # per sample
    tol_p: np.ndarray
    tol_loss: float     # of the batch's summed loss
    inv: np.ndarray     # unique row of every occurrence
    occ: np.ndarray     # [n_occ, D] per-occurrence gradient rows
    cnt: np.ndarray


def gradient(keys, R_of, y, nf, k, T=np.float64, rng=None, mutant=None, dR_of=None) -> Grad:
    """One batch's forward and per-key gradient.  ``keys`` [B, F] uint64 (any
    EMPTY marker compares equal to ``EMPTY``), ``R_of(u)`` the rows [nu, D] of
    the sorted distinct keys, ``dR_of(u)`` a bound they are known to (a
    free-running reference).  The bound is computed in fp64 from the values
    of this evaluation, whatever ``T``."""
    nb, D = len(y), 1 + nf * k
    if mutant == "field_by_rank":  # an occurrence's field: its rank among the non-EMPTY entries
        order = np.argsort(keys == EMPTY, axis=1, kind="stable")
        keys = np.take_along_axis(keys, order, axis=1)
    mask = keys != EMPTY
    u, first, inv = np.unique(keys[mask], return_index=True, return_inverse=True)
    nu, cnt = len(u), np.bincount(inv, minlength=len(u))
    R = R_of(u).astype(T)
    X = np.zeros((nb, nf, D), T)
    X[mask] = R[inv]
    off = ~np.eye(nf, dtype=bool)
    if mutant == "diag_included":
        off = np.ones((nf, nf), bool)
    live = mask[:, :, None] & mask[:, None, :]
    if mutant == "empty_as_id0":  # an EMPTY partner read as row 0 instead of skipped
        X[~mask] = R[0]
        live = np.broadcast_to(mask[:, :, None], live.shape)
    M = live & off
    if mutant == "dup_no_self_pair":
        M = M & (keys[:, :, None] != keys[:, None, :])
    V = X[..., 1:].reshape(nb, nf, nf, k)
    Pt = V.transpose(0, 2, 1, 3)                     # Pt[s, i, j] = R_j[i]
    if mutant == "same_block":                       # the partner R_j[j]
        Pt = np.broadcast_to(V[:, np.arange(nf), np.arange(nf)][:, None], V.shape)
    Pm = Pt * M[..., None]
    half = T(1.0 if mutant == "pair_twice" else 0.5)
    wt = X[..., 0] * mask
    pt = (half * V) * Pm
    if rng is None:
        z = wt.sum(1) + pt.sum((1, 2, 3))
    else:
        z = _kernel_sum(np.concatenate([wt, pt.reshape(nb, -1)], axis=1), geometry(nf, k)[1], rng)
    yy = y.astype(T)
    p = T(1) / (T(1) + np.exp(-z))
    g = p - yy
    loss = np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z))) - yy * z
    Go = np.empty((nb, nf, D), T)
    Go[..., 0] = g[:, None] * mask
    Go[..., 1:] = (g[:, None, None, None] * Pm).reshape(nb, nf, nf * k)
    if mutant == "dup_once":  # a key at two columns of a sample: the first column's gradient only
        later = (np.tril(keys[:, :, None] == keys[:, None, :], -1)).any(2)
        Go[later & mask] = 0
    occ = Go[mask]
    keep = np.ones(len(inv), bool)
    if mutant == "drop_65th":
        keep = _occ_rank(inv) != 64
    G = np.zeros((nu, D), T)
    order = np.nonzero(keep)[0] if rng is None else rng.permutation(np.nonzero(keep)[0])
    np.add.at(G, inv[order], occ[order])
    if mutant == "w_once_per_key":
        G[:, 0] = occ[first, 0]
    # ---- the bound, in fp64 (module docstring)
    z64, ag = z.astype(np.float64), np.abs(g.astype(np.float64))
    Bo = np.empty((nb, nf, D))
    Bo[..., 0] = mask
    Bo[..., 1:] = np.abs(Pm.astype(np.float64)).reshape(nb, nf, nf * k)
    Az = np.abs(wt.astype(np.float64)).sum(1) + np.abs(pt.astype(np.float64)).sum((1, 2, 3))
    dz = depth(nf, k) * U32 * Az
    if dR_of is not None:  # rows known to dR: first order through the forward
        dX = np.zeros((nb, nf, D))
        dX[mask] = dR_of(u)[inv]
        dPt = dX[..., 1:].reshape(nb, nf, nf, k).transpose(0, 2, 1, 3) * M[..., None]
        dzc = (dX[..., 0] * mask).sum(1) + (np.abs(V.astype(np.float64)) * dPt).sum((1, 2, 3))
        carry = (ag[:, None, None, None] * dPt).reshape(nb, nf, nf * k)
        carry = np.concatenate([np.zeros((nb, nf, 1)), carry], axis=2) + 0.25 * dzc[:, None, None] * Bo
    rel = ag * (U_G + (1 - ag) * dz) + U_A
    S = ag[:, None, None] * Bo
    per = rel[:, None, None] * Bo + U32 * S
    if dR_of is not None:
        per = per + carry
    eG, Ssum = np.zeros((nu, D)), np.zeros((nu, D))
    np.add.at(eG, inv, per[mask])
    np.add.at(Ssum, inv, S[mask])
    eG += cnt[:, None] * U32 * Ssum
    p64 = p.astype(np.float64)
    tol_p = SAFETY * (p64 * (1 - p64) * (dz + 2 * U32 * np.abs(z64)) + np.minimum(p64, 1 - p64) * U_G
                      + U_A)
    l64 = loss.astype(np.float64)
    e = np.exp(-np.abs(z64))
    el = (ag * dz + e / (1 + e) * (U_G + 2 * U32 * np.abs(z64)) + 4 * U32
          + 2 * U32 * (np.maximum(z64, 0) + np.abs(y * z64) + l64))
    blocks = -(-nb // (256 // geometry(nf, k)[1]))
    tol_loss = SAFETY * (el.sum() + (9 + -(-blocks // 256) + 16) * U32 * l64.sum())
    return Grad(u, G, eG, z, p, loss, tol_p, float(tol_loss), inv, occ, cnt)


def key_gradient(uid: np.ndarray, rows: np.ndarray, y: np.ndarray, k: int) -> Grad:
    """The fp64 gradient rows of one batch and their bound, for the
    kernel-level tests: ``uid`` [B, F] is each occurrence's unique row (-1 or
    0xFFFFFFFF: none), ``rows`` [n, 1 + F K] the unique rows.  ``G`` / ``eG``
    / ``cnt`` are per row of ``rows`` (rows with no occurrence: 0)."""
    uid = np.asarray(uid).astype(np.int64)
    none = (uid < 0) | (uid == 0xFFFFFFFF)
    keys = np.where(none, EMPTY, uid.astype(np.uint64))
    r = gradient(keys, lambda u: rows[u.astype(np.int64)], y, uid.shape[1], k)
    full = [np.zeros((len(rows),) + a.shape[1:], a.dtype) for a in (r.G, r.eG, r.cnt)]
    for f, a in zip(full, (r.G, r.eG, r.cnt)):
        f[r.u.astype(np.int64)] = a
    r.G, r.eG, r.cnt = full
    return r


def step_bound(opt: str, lr: float, x, h, G, eG, dx=0.0):
    """(x', h', tol_x, tol_h, ill) of one update in fp64: ``_opt_oracle``'s
    propagation of eG (and of a carried dx), times SAFETY; ill-conditioned
    coordinates bounded monotonically in G (module docstring)."""
    hy = _opt.Hyper(opt, lr=lr, eps=EPS).f32()
    ada = opt == "adagrad"
    run = lambda g: _opt.step(hy, _opt.N(x, dx), _opt.N(h, 0.0) if ada else None, None, g)  # noqa: E731
    w, s1, _ = run(_opt.N(G, eG))
    tol_x = SAFETY * w.e
    tol_h = SAFETY * s1.e if ada else np.zeros_like(tol_x)
    ill = ~np.isfinite(tol_x)
    if ada:
        ill |= eG > 0.1 * np.sqrt(s1.v + EPS)
    if ill.any():
        w0 = run(_opt.N(G, 0.0))[0]
        lo, hi = run(_opt.N(G - eG, 0.0))[0].v, run(_opt.N(G + eG, 0.0))[0].v
        mono = SAFETY * w0.e + np.maximum(np.abs(lo - w.v), np.abs(hi - w.v))
        tol_x = np.where(ill, mono, tol_x)
    return w.v, (s1.v if ada else h), tol_x, tol_h, ill


class FFMOracle:
    """The FFM over a sorted key set.  ``dtype`` float64 is the reference;
    float32 with ``perm`` (a seed) emulates the kernel's arithmetic with
    every order permuted.  ``mutant`` plants one of ``MUTANTS``.  ``init_rows``:
    keys -> [n, D] initial parameters (else the host mirror of the normal
    initialiser at ``scale``); the state starts at 0."""

    def __init__(self, nf: int, k: int, optimizer: str = "adagrad", lr: float | None = None,
                 scale: float = 0.01, dtype=np.float64, perm: int | None = None,
                 mutant: str | None = None, init_rows=None, carry: bool = False,
                 state_init: float = 0.0):
        assert optimizer in LR and mutant in (None,) + MUTANTS
        self.nf, self.k, self.D = nf, k, 1 + nf * k
        self.opt = optimizer
        self.lr = float(np.float32(LR[optimizer] if lr is None else lr))
        self.T, self.mutant, self.scale, self.carry = dtype, mutant, scale, carry
        self.rng = np.random.default_rng(perm) if perm is not None else None
        self.init_rows, self.state_init = init_rows, state_init
        self.keys = np.empty(0, np.uint64)
        self.x = self.h = np.empty((0, self.D), dtype)
        self.dx = np.empty((0, self.D))
        self.ill, self.zmax, self.losses = 0, 0.0, []

    def _init(self, new):
        from swiftsnails_amd.ops.optim import InitConfig, init_reference

        if self.init_rows is not None:
            return np.asarray(self.init_rows(new))
        return init_reference(InitConfig("normal", self.scale, 0.0), new, self.D, self.D)

    def _insert(self, u: np.ndarray) -> np.ndarray:
        pos = np.searchsorted(self.keys, u)
        hit = pos < len(self.keys)
        hit[hit] = self.keys[pos[hit]] == u[hit]
        new = u[~hit]
        if len(new):
            keys = np.concatenate([self.keys, new])
            order = np.argsort(keys)
            z = np.zeros((len(new), self.D))
            self.keys = keys[order]
            self.x = np.concatenate([self.x, self._init(new).astype(self.T)])[order]
            self.h = np.concatenate([self.h, (z + self.state_init).astype(self.T)])[order]
            self.dx = np.concatenate([self.dx, z])[order]
            pos = np.searchsorted(self.keys, u)
        return pos

    def rebase(self, keys, x, h) -> None:
        """Take (keys sorted and distinct, x, h) as the state, exactly."""
        self.keys = keys.copy()
        self.x, self.h = x.astype(self.T), h.astype(self.T)
        self.dx = np.zeros(self.x.shape)

    def step(self, keys: np.ndarray, y: np.ndarray, pulled=None) -> Grad:
        """One round on ``keys`` [B, F] / ``y``; ``pulled`` ([distinct keys of
        the batch sorted, D]): the rows the gradient is computed from where
        they are not the state (a replayed pull-ahead round).  Leaves
        ``pos`` / ``tol_x`` / ``tol_h`` of the batch's keys."""
        mask = keys != EMPTY
        pos = self._insert(np.unique(keys[mask]))
        r = gradient(keys, (lambda u: self.x[pos]) if pulled is None else (lambda u: pulled), y,
                     self.nf, self.k, self.T, self.rng, self.mutant,
                     (lambda u: self.dx[pos]) if self.carry else None)
        self.losses.append(r.loss.astype(np.float64))
        self.zmax = max(self.zmax, float(np.abs(r.z).max()))
        x, h = self.x[pos], self.h[pos]
        G64 = r.G.astype(np.float64)
        xr, hr, tol_x, tol_h, ill = step_bound(self.opt, self.lr, x.astype(np.float64),
                                               h.astype(np.float64), G64, r.eG,
                                               self.dx[pos] if self.carry else 0.0)
        if self.mutant == "update_per_occurrence":
            x, h = self._per_occurrence(x, h, r.inv, r.occ)
        elif self.T is np.float64:
            x, h = xr, hr
        else:
            x, h = update(self.opt, self.lr, x, h, r.G, self.T)
        self.x[pos], self.h[pos] = x, h
        self.ill += int(ill.any(1).sum())
        self.pos, self.tol_x, self.tol_h = pos, tol_x, tol_h
        if self.carry:
            self.dx[pos] = tol_x / SAFETY
        return r

    def _per_occurrence(self, x, h, inv, occ):
        """The mutant update: once per occurrence, in occurrence order."""
        rank = _occ_rank(inv)
        x, h, lr = x.copy(), h.copy(), self.T(self.lr)
        for r in range(rank.max() + 1):
            sel = np.nonzero(rank == r)[0]
            kk, t = inv[sel], occ[sel]
            if self.opt == "adagrad":
                h[kk] += t * t
                x[kk] -= lr * t / np.sqrt(h[kk] + self.T(EPS))
            else:
                x[kk] -= lr * t
        return x, h


def state_init(optimizer: str, row_dtype: str = "fp32") -> float:
    """The initial AdaGrad state of the planted rows as a table holds it."""
    if optimizer != "adagrad":
        return 0.0
    s = np.float32(STATE_INIT)
    if row_dtype == "bf16":  # round to nearest even
        b = s.view(np.uint32).astype(np.uint64)
        s = np.uint32((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).view(np.float32)
    return float(s)


def run(name: str, optimizer: str, world: int = 1, **kw) -> FFMOracle:
    kw.setdefault("state_init", state_init(optimizer))
    orc = FFMOracle(F[name], K[name], optimizer, scale=INIT_SCALE[name], **kw)
    for bk, y in batches(name, world):
        orc.step(bk, y)
    return orc


@functools.lru_cache(maxsize=None)
def reference(name: str, optimizer: str, world: int = 1) -> FFMOracle:
    """The free-running fp64 reference of a data set from the host mirror of
    the initialiser, computed once and shared."""
    return run(name, optimizer, world)


def free_running(name: str, init_rows, world: int = 1, source=None, nf=None, k=None, lr=None):
    """The free-running SGD reference with its carried bound: (keys, x,
    tol_x).  ``source``: the batches, where they are not a data set's."""
    orc = FFMOracle(nf or F[name], k or K[name], "sgd", lr=lr, init_rows=init_rows, carry=True)
    for bk, y in (source if source is not None else batches(name, world)):
        orc.step(bk, y)
    return orc.keys, orc.x, SAFETY * orc.dx


class Stepwise:
    """Holds a model under test to the oracle one step at a time: before each
    step the oracle takes the model's own state, computes the step in fp64
    with this step's bound, and the model's state after it must sit within
    the bound for every key the batch touched and be bit-identical for every
    other.  ``rx`` / ``rh`` / ``rl``: the largest |model - oracle| / bound
    (parameters, state, summed loss); ``out``: coordinates outside."""

    def __init__(self, nf: int, k: int, optimizer: str, lr: float | None = None, init_rows=None,
                 scale: float = 0.01, state_init: float = 0.0):
        self.orc = FFMOracle(nf, k, optimizer, lr=lr, init_rows=init_rows, scale=scale,
                             state_init=state_init)
        self.keys = np.empty(0, np.uint64)
        self.x = self.h = np.empty((0, self.orc.D))
        self.rx = self.rh = self.rl = 0.0
        self.out = 0
        self.outside_keys = np.empty(0, np.uint64)

    @property
    def ill(self) -> int:
        return self.orc.ill

    @property
    def zmax(self) -> float:
        return self.orc.zmax

    def step(self, bkeys, y, keys, x, h=None, pulled=None, loss=None, compare=True):
        """One step on the batch; (``keys``, ``x``, ``h``): the model's state
        after it (any order, each key once); ``loss``: its summed loss.
        ``compare=False``: the key set, the untouched rows and the oracle's
        step only (the caller holds the values itself: bf16 rows)."""
        o = self.orc
        o.rebase(self.keys, self.x, self.h)
        r = o.step(bkeys, y, pulled=pulled)
        order = np.argsort(keys)
        keys, x = keys[order], x[order].astype(np.float64)
        h = h[order].astype(np.float64) if h is not None else np.zeros_like(x)
        assert len(keys) == len(o.keys) and np.array_equal(keys, o.keys), (len(keys), len(o.keys))
        same = np.ones(len(keys), bool)
        same[o.pos] = False
        assert np.array_equal(x[same], o.x[same]) and np.array_equal(h[same], o.h[same])
        self.last = (o.pos, o.x[o.pos], o.h[o.pos], o.tol_x, o.tol_h)
        if compare:
            with np.errstate(divide="ignore", invalid="ignore"):
                dx, dh = np.abs(x[o.pos] - o.x[o.pos]), np.abs(h[o.pos] - o.h[o.pos])
                rx = np.where(dx == 0, 0.0, dx / o.tol_x)
                rh = np.where(dh == 0, 0.0, dh / o.tol_h)
            self.rx, self.rh = max(self.rx, float(rx.max())), max(self.rh, float(rh.max()))
            self.out += int((rx > 1).sum() + (rh > 1).sum())
            bad = ((rx > 1) | (rh > 1)).any(1)
            self.outside_keys = np.union1d(self.outside_keys, keys[o.pos[bad]])
        if loss is not None:
            self.rl = max(self.rl, abs(loss - r.loss.sum()) / r.tol_loss)
        self.keys, self.x, self.h = keys, x, h
        return r


def stepwise(name: str, optimizer: str, world: int = 1, steps: int = STEPS, **kw) -> Stepwise:
    """A free-running model (the oracle in fp32, or with a mutant) held to the
    oracle step by step."""
    nf, k, s = F[name], K[name], INIT_SCALE[name]
    h0 = kw.pop("state_init", state_init(optimizer))
    model = FFMOracle(nf, k, optimizer, scale=s, state_init=h0, **kw)
    sw = Stepwise(nf, k, optimizer, scale=s, state_init=h0)
    for bk, y in batches(name, world, steps):
        r = model.step(bk, y)
        sw.step(bk, y, model.keys, model.x, model.h, loss=float(r.loss.astype(np.float64).sum()))
    sw.model = model
    return sw


# Key-steps of the fp64 reference that are ill-conditioned when AdaGrad's state
# starts at 0 (host mirror of the initialiser, world 1): the first steps of keys
# with 13..350 occurrences whose |G| cancels.  They are bounded monotonically in
# G; the state-0 cases assert the count, so the fallback cannot spread unseen.
ILL_FROM_STATE_0 = {"ffm_mid": 0, "ffm_wide": 7, "ffm_small": 0}
