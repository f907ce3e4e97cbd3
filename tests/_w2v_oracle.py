"""A high-precision word2vec (SGNS) reference with an error bound, and its data.

Built like ``_fm_oracle.py`` and sharing what fits: the optimizer update and
its bound (``_lr_oracle.update`` / ``update_bound``), ``U32``, ``EPS`` and the
occurrence ranks.  Nothing here comes from the engine except ``init_reference``
(the host mirror of the key-seeded initialiser, bit-exact for the uniform
initialiser used here) and the ``W2VLayout`` key layout ``PlantedW2V`` derives
from.

The model (``W2VOracle``), mirroring ``models/word2vec.py``
----------------------------------------------------------
One table of ``dim``-float rows; input vectors are keyed by the word id,
output vectors by ``id | 1 << 40`` (``OUT``).  Three objectives:

* ``window`` / ``shared``: keys = [B centers | R = B + 2W run positions |
  tiles x 64 negatives], one meta word per run position (``ss/w2v_window.h``).
  Center t (run position t + W) pairs with position q iff both are unmasked,
  carry the same sentence tag and 0 < |q - t - W| <= b(center).  With n_t the
  center's pair count, per tile of 64 centers and its 64 negatives

      S+ = V U^T          G+ = sigmoid(S+) - 1 on the pairs, 0 elsewhere
      S- = V N^T          G- = (n_t K / 64) sigmoid(S-), 0 for n_t = 0
      gV = G+ U + G- N    gU = G+^T V    gN = G-^T V
      loss = sum softplus(-S+) + sum (n_t K / 64) softplus(S-)

  a center without pairs does not train (its row is not even read).
* ``pairs`` / ``shared``: keys = [B centers | B x 2W contexts | tiles x 64
  negatives]; every (center, context) is a pair, the negatives weigh
  ``2W K / 64``.
* ``window`` / ``per_pair``: keys = [B centers | R run positions | B x 2W x K
  negatives]; every valid pair (t, o) has its own K negatives, ``g+ =
  sigmoid(v.u) - 1``, ``g-_k = sigmoid(v.n_k)``.

Gradients are summed per distinct key over the whole batch (a key that is a
run position and a negative gets both), over the union of the ranks' batches
at world > 1, and one SGD / AdaGrad update per key follows (``ss/optim.h``).

Two evaluations of the shared-negative objectives
-------------------------------------------------
``exact`` is plain fp64.  ``as_built`` is fp64 arithmetic on the operands the
MFMA tile sees, every rounding where the kernel has it (``f2bf``, to nearest
even):

* ``k_w2v_win_bf16``: V, U and N rounded to bf16 before every GEMM (scores
  and gradients); G+ and G- rounded to bf16 after the fp32 sigmoid and the
  fp32 product with ``n_t K / 64``; the loss from the unrounded fp32 scores.
* ``k_w2v_sgns_bf16`` (pairs layout, ``SS_W2V_MFMA=bf16``): center and
  negative rows and ``neg_scale sigmoid(S)`` rounded; the positive pairs (dot
  products, ``g+``, ``g+ v``, ``g+ x``) stay fp32.

The engine is gated on ``as_built`` wherever a bf16 tile runs; the fp32 tile
(``SS_W2V_MFMA=f32``) and the per-pair kernels on ``exact``.  ``exact -
as_built`` is the modelling error of the bf16 tile, reported, not a gate.

The bound of one step (per key and coordinate, ``Grad.eG``)
------------------------------------------------------------
u = 2^-24.  Every gradient coordinate is a sum of products ``g_e x_ed`` (a
score gradient times a row coordinate).  With A = sum |g_e x_ed|:

    eG = sum_e dg_e |x_ed|  +  (L + c + 1) u A

* ``L`` is the kernel's accumulation length of the row (window tile: 96 + 64
  products for gV, 64 + 1 for gU and its tail row, 64 for gN; pairs tile:
  64 + 2W + 4; per-pair: 2W (1 + K) + 1, 2W + 1 and 1), ``c`` the number of
  occurrence (and tail) rows summed into the key: ``n u sum |terms|`` for any
  fp32 summation order of n terms.  In the bf16 GEMMs the products are exact
  (8 x 8 significand bits), so only the accumulation rounds.
* ``dg_e`` (``exact`` paths) is the fp32 evaluation error of the score
  gradient.  The kernels compute ``1 / (1 + __expf(-s))`` from a score known
  to ``eS = n u sum |v_d u_d|`` (n = D for the MFMA chains, D/64 + 7 for a
  lane-strided dot product with six shuffle adds):

      dsig(s) = p (1 - p) (eS + (2 + |s|) 2^-23) + 2 u

  (``__expf`` is the hardware exp2 of ``s log2 e``: 1 ulp of the result, and
  the argument's two roundings move e^-s by |s| 2^-23 relative, as
  ``_lr_oracle.py`` derives; a relative error r of e^-s moves p by p (1 - p) r;
  ``1 + e`` and the division round p by 1.5 u absolutely (``_fm_oracle.py``),
  ``p - 1`` by u / 2 more where p < 1/2); the weight's product adds u |g|.
* ``as_built``: an element of G+ / G- that the device rounds to the same bf16
  number as the oracle contributes *no* error at all, so ``dg_e = 0``; one
  whose fp64 value lies within ``dsig`` (times the weight) of a bf16 rounding
  midpoint may round the other way on the device.  The oracle flags these.
  A flagged element has exactly two possible device values, so with k of
  them the device's gradient is one of 2^k candidates, each with the bound
  above and **no widening**.  The candidate is found, not enumerated: a
  flipped element (t, q) adds ``delta U_q`` to its center's row and ``delta
  V_t`` to its context's (or negative's) row, a known pair of D-vectors, so
  the flipped subset is decoded from the observed gradient by greedy descent
  on the squared residual (``decode_flips``; the gradient is observed
  directly in the kernel tests, and through the step elsewhere: AdaGrad's
  state moves by exactly G^2, SGD's parameters by lr G).  One choice per
  element then holds for all D coordinates and both rows it feeds, and every
  coordinate is asserted against that one candidate at the tight bound.  A
  wrong decode can only fail the test, never pass a gradient that is not a
  candidate.  The share of widened coordinates is therefore zero.
  Compact bf16 rows cannot be decoded (stochastic rounding to 2^-8 swamps a
  flip, which moves a parameter by ~3e-5); there the stored value must be a
  bf16 neighbour of *some* candidate.  Neighbour intervals of adjacent values
  share their end points, so the union over the candidates is exactly the
  neighbour interval of the candidates' hull ``ref +- (tol + sum_flagged ulp
  |x|)``: the same candidate rule, evaluated in closed form (``Grad.hull``).

The loss: every term's score error, 4 u max(1, term) for softplus in fp32, and
64 u sum |terms| for the summation (lanes, shuffles, the sharded counter).

    adagrad:  dx = max |x(G +- eG) - x(G)|,  dh = 2 |G| eG + eG^2
    sgd:      dx = lr eG
    tol_x = 1e-6 + 1e-4 |x| + dx      tol_h = 1e-7 + 1e-4 h + dh

The relative and absolute terms are the LR / FM helpers'.  Their first-order
``dx = lr eG / sqrt(h_after + eps)`` needs a rule for ill-conditioned
key-steps (``eG > 0.1 sqrt(h_after + eps)``), and with rows of 32 to 128
coordinates, hundreds of keys and a worst-case ``eG`` nearly every word2vec
case has a few (0 to 11 of ~1e5 coordinate-steps: a coordinate whose summed
gradient happens to be below 1e-4).  Changing seeds until none is left in
any of fifty cases would fit the data to the rule.  So the step is bounded
without linearising: the AdaGrad step ``x(G) = x - lr G / sqrt(h + G^2 +
eps)`` is monotone in G, hence for a device gradient anywhere in ``G +- eG``
the parameter lies between ``x(G - eG)`` and ``x(G + eG)`` (evaluated with
the same ``update``), which is sound for every eG and excuses no key.  Where
the step is well conditioned the two agree to first order.  ``ill`` still
counts the rule's key-steps, as a figure.

The model is held one step at a time (``Stepwise``; ``_fm_oracle.py`` says
why a carried AdaGrad bound is not tried again): keys the batch did not
touch, and keys whose every gradient term is structurally zero (masked
positions, centers without pairs, negatives of pairs that are not valid),
must be bit-identical.

Departures from the issue, from the arithmetic alone
----------------------------------------------------
* The planted occurrence counts 1, 2, 31, 32, 33, 64, 65 *and* a key with at
  least 300 occurrences need 528 output-namespace slots; a window batch of
  B = 200, W = 5 has 210 + 256 = 466.  So the counts alternate: even steps
  carry 1 .. 65, odd steps the 300-occurrence key beside 1 .. 33 (``plan``).
  Smaller batches carry the counts that fit 90 % of their slots.
* The flip window.  The issue estimates 3e-5 flagged elements per element,
  which counts the sigmoid's own rounding only.  The window that is *sound*
  also holds the score's fp32 accumulation error (D u sum |v_d u_d|, about
  1e-5 at D = 64 against a bf16 spacing of 2e-3 to 4e-3) and flags 0.05-3 %
  of the elements.  That is why flagged elements are settled by decoding
  (above) instead of widening what they feed: widening would have loosened
  5-19 % of the window layout's coordinates.  The cap on widened coordinates
  (``WIDE_CAP``, the issue's 1 %) is asserted over all eight steps of every
  case and met with a share of zero.

Measured on the CPU (``test_w2v_oracle_cpu.py``)
-----------------------------------------------
The fp32 emulation (three permuted orders, bf16 operands where the tile has
them), step by step, max |fp32 - fp64| / tol over every data set and dim 32 /
64 / 128: x 0.004-0.057, h 0.010-0.057.  The gradient alone against ``eG``,
flagged elements settled: 0.04-0.07 (window), 0.21-0.26 (pairs), 0.21-0.36
(per-pair); the loss at most 0.002 of its bound.  Every mutant is rejected
with a max
ratio of 1.9e3 and more under AdaGrad and 1.8e2 and more under SGD
(``per_item_update`` is no mutant under SGD, which is linear in the gradient);
``docs/TESTING.md`` has the table.  ``exact - as_built``: 2.0e-3 to 2.3e-3
median relative in the window layout (about a hundred times ``eG``), the
bf16 tile's modelling error.  On the MI355X every path sits at the
emulation's floor (``test_gpu_w2v_paths_oracle.py`` has the table).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from _fm_oracle import _occ_rank
from _lr_oracle import EPS, U32, update, update_bound
from swiftsnails_amd.models.word2vec import W2VLayout

OUT_BIT = 40
OUT = np.uint64(1 << OUT_BIT)
TILE = NEG = 64
STEPS = 8
CHUNK = 32            # occurrences per reduce item (kOsCh)
LR = {"adagrad": 0.05, "sgd": 5e-4}
WIDE_CAP = 0.01       # widened coordinates per case (the issue's cap; the share is zero)
COUNTS = (1, 2, 31, 32, 33, 64, 65)
HOT = 300
MUTANTS = ("nt_plus_one", "nt_of_neighbour", "window_of_context", "cross_sentence",
           "drop_33rd", "tail_twice", "pp_wrong_center", "per_item_update", "g_truncated")


def init_scale(dim: int) -> float:
    """Uniform ``(u - 0.5) s`` rows whose scores v.u have a standard deviation
    of 1: sqrt(D) s^2 / 12 = 1."""
    return float(np.sqrt(12 / np.sqrt(dim)))


# ------------------------------------------------------------------- bf16
def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)


def bf16(x):
    """``f2bf``: the fp32 value of x rounded to bf16, to nearest even."""
    u = _bits(x)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_trunc(x):
    return (_bits(x) & np.uint64(0xFFFF0000)).astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_ulp(x):
    """Spacing of the bf16 numbers at |x| (8 significand bits); 0 at 0."""
    _, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.where(np.asarray(x) != 0, np.ldexp(1.0, e - 8), 0.0)


def near_midpoint(g, d):
    """|g| lies within d of the midpoint of its two bf16 neighbours."""
    mid = np.abs(bf16_trunc(g)) + 0.5 * bf16_ulp(g)
    return np.abs(np.abs(np.asarray(g, np.float64)) - mid) <= d


def flip_delta(g, rounded):
    """What the other bf16 neighbour of g adds to ``rounded`` (g's rounding)."""
    lo = np.abs(bf16_trunc(g))
    return np.sign(np.asarray(g, np.float64)) * (2 * lo + bf16_ulp(g) - 2 * np.abs(rounded))


def decode_flips(R, kA, kB, vA, vB, eG=None):
    """Which flagged elements rounded the other way: the subset f minimising
    ``|R - sum_f (vA at row kA + vB at row kB)|^2`` by greedy descent, with
    pairs of toggles to leave a local minimum (R
    [rows, D]: observed minus oracle gradient; a flagged element adds vA to
    row kA and vB to row kB when flipped; with ``eG`` the residual is weighed
    by the bound, 1 / eG^2, so a row with a loose bound does not outvote one
    with a tight bound).  Returns (f, the correction
    [rows, D]).  The answer is only a proposal: what is asserted afterwards is
    every coordinate's ordinary bound against the oracle with exactly these
    elements flipped, i.e. against one of the 2^k candidates."""
    m = len(kA)
    f, C = np.zeros(m, bool), np.zeros_like(R)
    if not m:
        return f, C
    R = R.copy()
    w = np.ones_like(R) if eG is None else 1.0 / np.maximum(eG, 1e-12) ** 2
    wA, wB = w[kA] * vA, w[kB] * vB
    nrm = (wA * vA).sum(1) + (wB * vB).sum(1)

    def toggle(e, s):
        R[kA[e]] -= s * vA[e]
        R[kB[e]] -= s * vB[e]
        C[kA[e]] += s * vA[e]
        C[kB[e]] += s * vB[e]
        f[e] = ~f[e]

    def gains():
        s = np.where(f, -1.0, 1.0)
        return s, 2 * s * ((R[kA] * wA).sum(1) + (R[kB] * wB).sum(1)) - nrm

    def descend():
        for _ in range(4 * m):
            s, gain = gains()
            e = int(np.argmax(gain))
            if gain[e] <= 0:
                return
            toggle(e, s[e])

    descend()
    for _ in range(32):   # out of a local minimum: the best pair of toggles among the
        bad = (R * R * w > 0.25).any(1)   # elements that feed a row still off by half its bound
        S = np.nonzero(bad[kA] | bad[kB])[0][:256]
        if not len(S):
            break
        s, gain = gains()
        best, pair = 0.0, None
        for a, i in enumerate(S):
            J = S[a + 1:]
            cross = (((kA[J] == kA[i])[:, None] * wA[J] * vA[i]).sum(1)
                     + ((kB[J] == kB[i])[:, None] * wB[J] * vB[i]).sum(1)
                     + ((kA[J] == kB[i])[:, None] * wA[J] * vB[i]).sum(1)
                     + ((kB[J] == kA[i])[:, None] * wB[J] * vA[i]).sum(1))
            g2 = gain[i] + gain[J] - 2 * s[i] * s[J] * cross
            if len(J) and g2.max() > best:
                best, pair = float(g2.max()), (i, int(J[int(np.argmax(g2))]))
        if pair is None:
            break
        toggle(pair[0], s[pair[0]])
        toggle(pair[1], s[pair[1]])
        descend()
    return f, C


def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def _sp(z):
    return np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))


def dsig(s, eS):
    """fp32 evaluation error of sigmoid(s) (and of sigmoid(s) - 1) from a
    score known to eS (module docstring)."""
    s = np.asarray(s, np.float64)
    p = _sig(s)
    return p * (1 - p) * (eS + (2 + np.abs(s)) * 2.0 ** -23) + 2 * U32


# ------------------------------------------------------------------- layout
@dataclass(frozen=True)
class Spec:
    layout: str          # window | pairs
    neg: str             # shared | per_pair
    B: int
    W: int
    K: int = 5

    @property
    def R(self):
        return self.B + 2 * self.W

    @property
    def C(self):
        return 2 * self.W

    @property
    def tiles(self):
        return (self.B + TILE - 1) // TILE

    @property
    def n_neg(self):
        return self.B * self.C * self.K if self.neg == "per_pair" else self.tiles * NEG

    @property
    def n_ctx(self):
        return self.R if self.layout == "window" else self.B * self.C

    @property
    def n_keys(self):
        return self.B + self.n_ctx + self.n_neg


def pairs_mask(meta, B, W, mutant=None):
    """Valid pairs [B, B + 2W] of a window run (``ss/w2v_window.h``)."""
    m = meta.astype(np.int64)
    c, q = m[W:W + B][:, None], m[None, :]
    d = np.abs(np.arange(B + 2 * W)[None, :] - (np.arange(B)[:, None] + W))
    b = (q & 15) if mutant == "window_of_context" else (c & 15)
    same = ((c >> 4) == (q >> 4)) | (mutant == "cross_sentence")
    return (c >= 0) & (q >= 0) & same & (d != 0) & (d <= b) & (d <= W)


def offsets(W):
    """Run offset of pair slot o (per-pair layout): -W .. -1, 1 .. W."""
    return np.array([o - W if o < W else o - W + 1 for o in range(2 * W)])


# ----------------------------------------------------------------- gradient
@dataclass
class Occ:
    """One batch's occurrence rows (one per key position) with the bound's
    ingredients, all [n_keys, D] but ``L`` [n_keys]."""
    G: np.ndarray
    E: np.ndarray      # sum dg_e |x_ed|
    A: np.ndarray      # sum |g_e x_ed|
    Wd: np.ndarray     # sum over flagged elements of ulp_bf16(g_e) |x_ed|
    L: np.ndarray
    extra: np.ndarray  # [n_keys] rows summed beside the occurrence row (the tail copy)
    loss: float
    eloss: float
    pairs: int
    smax: float = 0.0
    scores: np.ndarray | None = None   # every live score, positive pairs first (data-set checks)
    flagged: int = 0                   # flagged elements of G+ / G-
    elements: int = 0                  # live elements of G+ / G-
    Gtail: np.ndarray | None = None    # window layout: the part of G a tail row carries
    flips: tuple | None = None         # flagged elements: (rowA, rowB, vecA, vecB), decode_flips


class _Arith:
    """fp64 exactly enough, or fp32 with every sum in a permuted order (the
    emulation of the device arithmetic)."""

    def __init__(self, dtype=np.float64, perm=None):
        self.T = dtype
        self.rng = np.random.default_rng(perm) if perm is not None else None

    def mm(self, a, b):
        """a [n, k] @ b [k, m]."""
        if self.rng is None:
            return a @ b
        out = np.zeros((a.shape[0], b.shape[1]), self.T)
        for k in self.rng.permutation(a.shape[1]):
            out += a[:, k:k + 1] * b[k:k + 1, :]
        return out

    def dot_last(self, a, b):
        """sum over the last axis of a * b (broadcast), permuted in fp32."""
        if self.rng is None:
            return (a * b).sum(-1)
        out = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1], self.T)
        for d in self.rng.permutation(a.shape[-1]):
            out += a[..., d] * b[..., d]
        return out

    def sum_axis(self, a, axis):
        if self.rng is None:
            return a.sum(axis)
        a = np.moveaxis(a, axis, 0)
        out = np.zeros(a.shape[1:], self.T)
        for i in self.rng.permutation(a.shape[0]):
            out += a[i]
        return out

    def sig(self, z):
        return self.T(1) / (self.T(1) + np.exp(-z))


def _round(mode, mutant):
    """(rounding of the tile's row operands, rounding of its score gradients)."""
    if mode == "exact":
        return (lambda x: np.asarray(x, np.float64)), (lambda x: x)
    return bf16, (bf16_trunc if mutant == "g_truncated" else bf16)


def grad_window(sp: Spec, X, meta, mode="as_built", mutant=None, ar: _Arith | None = None):
    """The window layout with shared negatives (``k_w2v_win_bf16``): ``X``
    [n_keys, D] the row of every key position."""
    ar = ar or _Arith()
    T, f64 = ar.T, np.float64
    B, W, R, D = sp.B, sp.W, sp.R, X.shape[1]
    rr, rg = _round(mode, mutant)
    emu = ar.rng is not None
    cast = (lambda x: x.astype(T)) if emu else (lambda x: x)
    mask = pairs_mask(meta, B, W, mutant)
    n = mask.sum(1)
    train = n > 0
    unm = meta >= 0
    Vb = cast(rr(X[:B]) * train[:, None])
    Ub = cast(rr(X[B:B + R]) * unm[:, None])
    Nb = cast(rr(X[B + R:])).reshape(sp.tiles, NEG, D)
    nw = (n + train if mutant == "nt_plus_one" else
          np.roll(n, 1) if mutant == "nt_of_neighbour" else n)
    cw = (nw * (sp.K / NEG) * train).astype(T)
    Sp = ar.mm(Vb, Ub.T)
    Gp_raw = np.where(mask, ar.sig(Sp) - T(1), T(0))
    Sn = np.zeros((B, NEG), T)
    for t in range(sp.tiles):
        c = slice(t * TILE, min(B, (t + 1) * TILE))
        Sn[c] = ar.mm(Vb[c], Nb[t].T)
    Gn_raw = cw[:, None] * ar.sig(Sn) * train[:, None]
    Gp, Gn = cast(rg(Gp_raw)), cast(rg(Gn_raw))
    gV = ar.mm(Gp, Ub)
    gN = np.zeros((sp.tiles, NEG, D), T)
    for t in range(sp.tiles):
        c = slice(t * TILE, min(B, (t + 1) * TILE))
        gV[c] += ar.mm(Gn[c], Nb[t])
        gN[t] = ar.mm(Gn[c].T, Vb[c])
    gU = ar.mm(Gp.T, Vb)
    # the tail rows: position q >= 64 with q % 64 < 2W is also row 64 + q % 64
    # of the previous tile, whose part goes through the tail buffer
    q = np.arange(R)
    tail = (q >= TILE) & (q % TILE < 2 * W) & (q // TILE <= sp.tiles - 1)
    tmask = tail[None, :] & ((np.arange(B) // TILE)[:, None] == (q // TILE - 1)[None, :])
    Gtail = np.zeros((sp.n_keys, D), f64)
    Gtail[B:B + R] = (Gp * tmask).T.astype(f64) @ Vb.astype(f64)
    if mutant == "tail_twice":
        gU = gU + ar.mm((Gp * tmask).T, Vb)
    G = np.concatenate([gV, gU, gN.reshape(-1, D)]).astype(f64)
    # ---- the loss and the bound, from the reference's own quantities
    Sp64, Sn64, cw64 = Sp.astype(f64), Sn.astype(f64), cw.astype(f64)
    aV, aU, aN = np.abs(Vb).astype(f64), np.abs(Ub).astype(f64), np.abs(Nb).astype(f64)
    lp, ln = mask * _sp(-Sp64), train[:, None] * cw64[:, None] * _sp(Sn64)
    loss = lp.sum() + ln.sum()
    eSp = D * U32 * (aV @ aU.T)
    eSn = np.concatenate([D * U32 * (aV[t * TILE:(t + 1) * TILE] @ aN[t].T)
                          for t in range(sp.tiles)])
    live_n = train[:, None] & np.ones((1, NEG), bool)
    eloss = ((mask * (eSp + 4 * U32 * np.maximum(1, lp))).sum()
             + (live_n * cw64[:, None] * (eSn + 4 * U32 * np.maximum(1, _sp(Sn64)))).sum()
             + 64 * U32 * loss)
    dGp = mask * dsig(Sp64, eSp)
    dGn = live_n * (cw64[:, None] * dsig(Sn64, eSn) + U32 * np.abs(Gn_raw.astype(f64)))
    if mode == "exact":
        EP, EN = dGp, dGn
        WP, WN = np.zeros_like(dGp), np.zeros_like(dGn)
        flagged, flips = 0, None
    else:
        fP = mask & near_midpoint(Gp_raw.astype(f64), dGp)
        fN = live_n & near_midpoint(Gn_raw.astype(f64), dGn)
        WP, WN = fP * bf16_ulp(Gp_raw.astype(f64)), fN * bf16_ulp(Gn_raw.astype(f64))
        EP, EN = np.zeros_like(dGp), np.zeros_like(dGn)
        flagged = int(fP.sum() + fN.sum())
        # a flipped element (t, q) of G+ adds delta U_q to center t and delta V_t to
        # position q; (t, k) of G- adds delta N_k to center t and delta V_t to negative k
        tp, qp = np.nonzero(fP)
        tn, kn = np.nonzero(fN)
        dp = flip_delta(Gp_raw.astype(f64)[tp, qp], Gp.astype(f64)[tp, qp])
        dn = flip_delta(Gn_raw.astype(f64)[tn, kn], Gn.astype(f64)[tn, kn])
        V64, U64, N64 = Vb.astype(f64), Ub.astype(f64), Nb.astype(f64)
        flips = (np.concatenate([tp, tn]), np.concatenate([B + qp, B + R + (tn // TILE) * NEG + kn]),
                 np.concatenate([dp[:, None] * U64[qp], dn[:, None] * N64[tn // TILE, kn]]),
                 np.concatenate([dp[:, None] * V64[tp], dn[:, None] * V64[tn]]))
    aGp, aGn = np.abs(Gp).astype(f64), np.abs(Gn).astype(f64)

    def rows(P, Nn):
        """[n_keys, D] of sum |x_ed| weights: P [B, R] on G+, Nn [B, 64] on G-."""
        v = P @ aU
        nn = np.zeros((sp.tiles, NEG, D))
        for t in range(sp.tiles):
            c = slice(t * TILE, min(B, (t + 1) * TILE))
            v[c] += Nn[c] @ aN[t]
            nn[t] = Nn[c].T @ aV[c]
        return np.concatenate([v, P.T @ aV, nn.reshape(-1, D)])

    L = np.concatenate([np.full(B, 96 + 64), np.full(R, 64 + 1), np.full(sp.n_neg, 64)])
    extra = np.concatenate([np.zeros(B, int), tail.astype(int), np.zeros(sp.n_neg, int)])
    return Occ(G, rows(EP, EN), rows(aGp, aGn), rows(WP, WN), L, extra, float(loss),
               float(eloss), int(n.sum()), float(max(np.abs(Sp64[mask]).max(initial=0),
                                                     np.abs(Sn64[train]).max(initial=0))),
               np.concatenate([Sp64[mask], Sn64[train].reshape(-1)]), flagged,
               int(mask.sum() + live_n.sum()), Gtail, flips)


def grad_pairs(sp: Spec, X, mode="as_built", mutant=None, ar: _Arith | None = None,
               neg_scale=None):
    """The pairs layout (``k_w2v_sgns_bf16`` as_built, ``k_w2v_sgns`` exact);
    ``neg_scale``: the negatives' weight where it is not ``2W K / 64`` (the
    kernel-level tests)."""
    ar = ar or _Arith()
    T, f64 = ar.T, np.float64
    B, C, D = sp.B, sp.C, X.shape[1]
    rr, rg = _round(mode, mutant)
    emu = ar.rng is not None
    cast = (lambda x: x.astype(T)) if emu else (lambda x: x)
    ns = T(np.float32(C * sp.K / NEG if neg_scale is None else neg_scale))
    V, Xc = cast(X[:B]), cast(X[B:B + B * C]).reshape(B, C, D)
    Vb, Nb = cast(rr(X[:B])), cast(rr(X[B + B * C:])).reshape(sp.tiles, NEG, D)
    pos = ar.dot_last(V[:, None, :], Xc)
    gp = ar.sig(pos) - T(1)
    gX = gp[:, :, None] * V[:, None, :]
    gV = ar.sum_axis(gp[:, :, None] * Xc, 1)
    S = np.zeros((B, NEG), T)
    for t in range(sp.tiles):
        c = slice(t * TILE, min(B, (t + 1) * TILE))
        S[c] = ar.mm(Vb[c], Nb[t].T)
    G_raw = ns * ar.sig(S)
    Gb = cast(rg(G_raw))
    gN = np.zeros((sp.tiles, NEG, D), T)
    for t in range(sp.tiles):
        c = slice(t * TILE, min(B, (t + 1) * TILE))
        gV[c] = gV[c] + ar.mm(Gb[c], Nb[t])
        gN[t] = ar.mm(Gb[c].T, Vb[c])
    G = np.concatenate([gV, gX.reshape(-1, D), gN.reshape(-1, D)]).astype(f64)
    # ---- loss and bound
    pos64, S64 = pos.astype(f64), S.astype(f64)
    aV, aX = np.abs(X[:B]).astype(f64), np.abs(X[B:B + B * C]).astype(f64).reshape(B, C, D)
    aVb, aN = np.abs(Vb).astype(f64), np.abs(Nb).astype(f64)
    ldot = (D + 63) // 64 + 7
    epos = ldot * U32 * (aV[:, None, :] * aX).sum(-1)
    eS = np.concatenate([(D + 1) * U32 * (aVb[t * TILE:(t + 1) * TILE] @ aN[t].T)
                         for t in range(sp.tiles)])
    lp, ln = _sp(-pos64), float(ns) * _sp(S64)
    loss = lp.sum() + ln.sum()
    eloss = ((epos + 4 * U32 * np.maximum(1, lp)).sum()
             + (float(ns) * (eS + 4 * U32 * np.maximum(1, _sp(S64)))).sum() + 64 * U32 * loss)
    dgp = dsig(pos64, epos)
    dG = float(ns) * dsig(S64, eS) + U32 * np.abs(G_raw.astype(f64))
    if mode == "exact":
        EN, WN, flagged, flips = dG, np.zeros_like(dG), 0, None
    else:
        fN = near_midpoint(G_raw.astype(f64), dG)
        EN, WN, flagged = np.zeros_like(dG), fN * bf16_ulp(G_raw.astype(f64)), int(fN.sum())
        tn, kn = np.nonzero(fN)
        dn = flip_delta(G_raw.astype(f64)[tn, kn], Gb.astype(f64)[tn, kn])
        flips = (tn, B + B * C + (tn // TILE) * NEG + kn,
                 dn[:, None] * Nb.astype(f64)[tn // TILE, kn], dn[:, None] * Vb.astype(f64)[tn])
    agp, aG = np.abs(gp).astype(f64), np.abs(Gb).astype(f64)

    def rows(pp, Nn):
        """pp [B, C] on g+, Nn [B, 64] on the negatives' score gradients."""
        v = (pp[:, :, None] * aX).sum(1)
        nn = np.zeros((sp.tiles, NEG, D))
        for t in range(sp.tiles):
            c = slice(t * TILE, min(B, (t + 1) * TILE))
            v[c] += Nn[c] @ aN[t]
            nn[t] = Nn[c].T @ aVb[c]
        x = pp[:, :, None] * aV[:, None, :]
        return np.concatenate([v, x.reshape(-1, D), nn.reshape(-1, D)])

    L = np.concatenate([np.full(B, 64 + C + 4), np.full(B * C, 1), np.full(sp.n_neg, 64 + 1)])
    return Occ(G, rows(dgp, EN), rows(agp, aG), rows(np.zeros_like(dgp), WN), L,
               np.zeros(sp.n_keys, int), float(loss), float(eloss), B * C,
               float(max(np.abs(pos64).max(), np.abs(S64).max())),
               np.concatenate([pos64.reshape(-1), S64.reshape(-1)]), flagged,
               int(S64.size), None, flips)


def grad_per_pair(sp: Spec, X, meta, mutant=None, ar: _Arith | None = None):
    """Per-pair negatives (``k_w2v_pp`` / ``k_w2v_pp16`` / ``k_w2v_ppctx`` and
    the scaled rows of the reduce), plain fp32 on the device: exact only."""
    ar = ar or _Arith()
    T, f64 = ar.T, np.float64
    B, W, R, K, D = sp.B, sp.W, sp.R, sp.K, X.shape[1]
    P2 = 2 * W
    emu = ar.rng is not None
    X = X.astype(T) if emu else X
    qidx = np.arange(B)[:, None] + W + offsets(W)[None, :]
    m = pairs_mask(meta, B, W, mutant)[np.arange(B)[:, None], qidx]
    V, U = X[:B], X[B:B + R]
    N = X[B + R:].reshape(B, P2, K, D)
    Uc = U[qidx]
    s_p = ar.dot_last(V[:, None, :], Uc)
    s_n = ar.dot_last(V[:, None, None, :], N)
    gp = (ar.sig(s_p) - T(1)) * m
    gn = ar.sig(s_n) * m[:, :, None]
    gV = ar.sum_axis(gp[:, :, None] * Uc, 1) + ar.sum_axis(
        (gn[..., None] * N).reshape(B, P2 * K, D), 1)
    gU = np.zeros((R, D), T)
    np.add.at(gU, qidx.reshape(-1), (gp[:, :, None] * V[:, None, :]).reshape(-1, D))
    Vs = np.roll(V, 1, axis=0) if mutant == "pp_wrong_center" else V
    gN = gn[..., None] * Vs[:, None, None, :]
    G = np.concatenate([gV, gU, gN.reshape(-1, D)]).astype(f64)
    # ---- loss and bound
    sp64, sn64 = s_p.astype(f64), s_n.astype(f64)
    aV, aUc, aN = np.abs(V).astype(f64), np.abs(Uc).astype(f64), np.abs(N).astype(f64)
    ldot = (D + 63) // 64 + 7
    esp = ldot * U32 * (aV[:, None, :] * aUc).sum(-1)
    esn = ldot * U32 * (aV[:, None, None, :] * aN).sum(-1)
    lp, ln = m * _sp(-sp64), m[:, :, None] * _sp(sn64)
    loss = lp.sum() + ln.sum()
    eloss = ((m * (esp + 4 * U32 * np.maximum(1, lp))).sum()
             + (m[:, :, None] * (esn + 4 * U32 * np.maximum(1, ln))).sum() + 64 * U32 * loss)
    dgp, dgn = m * dsig(sp64, esp), m[:, :, None] * dsig(sn64, esn)
    agp, agn = np.abs(gp).astype(f64), np.abs(gn).astype(f64)

    def rows(pp, nn):
        v = (pp[:, :, None] * aUc).sum(1) + (nn[..., None] * aN).sum((1, 2))
        u = np.zeros((R, D))
        np.add.at(u, qidx.reshape(-1), (pp[:, :, None] * aV[:, None, :]).reshape(-1, D))
        return np.concatenate([v, u, (nn[..., None] * aV[:, None, None, :]).reshape(-1, D)])

    L = np.concatenate([np.full(B, P2 * (1 + K) + 1), np.full(R, P2 + 1), np.full(sp.n_neg, 1)])
    z = np.zeros((sp.n_keys, D))
    return Occ(G, rows(dgp, dgn), rows(agp, agn), z, L, np.zeros(sp.n_keys, int), float(loss),
               float(eloss), int(m.sum()),
               float(max(np.abs(sp64[m]).max(initial=0), np.abs(sn64[m]).max(initial=0))),
               np.concatenate([sp64[m], sn64[m].reshape(-1)]), 0, 0)


SHARDS = 256 * 32   # the loss counter's shards (``ops/table.py loss_buffer``)


def shard_sum_error(loss, n=SHARDS) -> float:
    """fp32 error of summing the loss counter's ``n`` non-negative shards on
    the device and dividing once: a reduction that adds up to 16 elements per
    thread in sequence and the threads' partial sums as a tree has chains of
    16 + log2(n) additions, each within u of the running sum, plus the
    division's u."""
    return (16 + int(np.ceil(np.log2(n))) + 1) * U32 * abs(float(loss))


def occ_bound(o: Occ) -> np.ndarray:
    """The bound of every occurrence row on its own [n_keys, D] (the
    kernel-level tests: every key position its own row; a window row's tail
    part arrives as one more addend)."""
    return o.E + (o.L + o.extra + 2)[:, None] * U32 * o.A


def settle_occ(o: Occ, G) -> tuple:
    """(o.G with the flagged elements flipped that the observed occurrence rows
    ``G`` say were, the number flipped)."""
    if o.flips is None:
        return o.G, 0
    f, C = decode_flips(np.asarray(G, np.float64) - o.G, *o.flips, eG=occ_bound(o))
    return o.G + C, int(f.sum())


def occurrence_rows(sp: Spec, X, meta, mode, mutant=None, ar=None) -> Occ:
    if sp.neg == "per_pair":
        return grad_per_pair(sp, X, meta, mutant, ar)
    if sp.layout == "window":
        return grad_window(sp, X, meta, mode, mutant, ar)
    return grad_pairs(sp, X, mode, mutant, ar)


@dataclass
class Grad:
    """A step's gradient per distinct key with its bound."""
    keys: np.ndarray     # sorted, distinct
    G: np.ndarray        # [n, D]
    eG: np.ndarray       # [n, D]
    wide: np.ndarray     # [n, D] bool: a flagged element feeds the coordinate
    zero: np.ndarray     # [n] bool: every term structurally zero
    cnt: np.ndarray      # [n] occurrences
    loss: np.ndarray     # [ranks]
    eloss: np.ndarray
    pairs: np.ndarray    # [ranks] positive pairs
    smax: float
    flagged: int
    elements: int
    inv: np.ndarray = field(repr=False, default=None)   # unique row of every key position
    occ: list = field(repr=False, default=None)
    flips: tuple = field(repr=False, default=None)      # (keyA, keyB, vecA, vecB) per flagged element
    hull: np.ndarray = field(repr=False, default=None)  # [n, D] sum over flagged of ulp |x| (bf16 rows)
    nflip: int = 0                                      # elements settled as flipped

    def settle(self, G_est):
        """Flip the flagged elements the observed per-key gradient says were."""
        if self.flips is not None:
            f, C = decode_flips(np.asarray(G_est, np.float64) - self.G, *self.flips, eG=self.eG)
            self.G, self.nflip = self.G + C, int(f.sum())
        return self


def key_gradient(sp: Spec, batches, rows_of, mode="as_built", mutant=None, ar=None) -> Grad:
    """Sum the occurrence rows of the ranks' batches (``[(keys, meta), ...]``)
    per distinct key; ``rows_of(u)``: the [n, D] rows of the sorted distinct
    keys ``u``."""
    allk = np.concatenate([k for k, _ in batches])
    u, inv = np.unique(allk, return_inverse=True)
    Rw = rows_of(u)
    nu, D = len(u), Rw.shape[1]
    occ, at = [], 0
    for k, meta in batches:
        occ.append(occurrence_rows(sp, Rw[inv[at:at + len(k)]], meta, mode, mutant, ar))
        at += len(k)
    cat = lambda f: np.concatenate([f(o) for o in occ])  # noqa: E731
    Gocc, E, A, Wd, L, extra = (cat(lambda o, n=n: getattr(o, n))
                                for n in ("G", "E", "A", "Wd", "L", "extra"))
    keep = np.ones(len(inv), bool)
    if mutant == "drop_33rd":
        keep = _occ_rank(inv) != CHUNK
    G = np.zeros((nu, D))
    if ar is not None and ar.rng is not None:
        order = ar.rng.permutation(np.nonzero(keep)[0])
        G = G.astype(ar.T)
        np.add.at(G, inv[order], Gocc[order].astype(ar.T))
        G = G.astype(np.float64)
    else:
        np.add.at(G, inv[keep], Gocc[keep])
    sA, sE, sW, sLA = (np.zeros((nu, D)) for _ in range(4))
    np.add.at(sA, inv, A)
    np.add.at(sE, inv, E)
    np.add.at(sW, inv, Wd)
    np.add.at(sLA, inv, L[:, None] * A)
    cnt = np.bincount(inv, minlength=nu)
    terms = cnt + np.bincount(inv, extra, minlength=nu)
    eG = sE + U32 * sLA + (terms + 1)[:, None] * U32 * sA
    flips, at = [], 0
    for o, (k, _) in zip(occ, batches):
        if o.flips is not None:
            flips.append((inv[at + o.flips[0]], inv[at + o.flips[1]], o.flips[2], o.flips[3]))
        at += len(k)
    flips = tuple(np.concatenate(x) for x in zip(*flips)) if flips else None
    # no coordinate is widened: flagged elements are settled (``settle``), not excused
    return Grad(u, G, eG, np.zeros((nu, D), bool), ~sA.any(1), cnt,
                np.array([o.loss for o in occ]),
                np.array([o.eloss for o in occ]), np.array([o.pairs for o in occ]),
                max(o.smax for o in occ), sum(o.flagged for o in occ),
                sum(o.elements for o in occ), inv, occ, flips, sW)


# -------------------------------------------------------------------- model
@dataclass
class Result:
    keys: np.ndarray
    x: np.ndarray
    h: np.ndarray
    tol_x: np.ndarray
    tol_h: np.ndarray
    touched: np.ndarray   # [n] bool: keys of the latest batch
    zero: np.ndarray      # [n] bool: touched, every gradient term structurally zero
    wide: np.ndarray      # [n, D] bool
    grad: Grad


class W2VOracle:
    """word2vec over a sorted key set.  ``dtype`` float64 is the reference;
    float32 with ``perm`` (a seed) is the emulation of the device arithmetic
    (fp32 accumulation in permuted orders, bf16 operands where ``mode`` is
    ``as_built``).  ``mutant`` plants one of ``MUTANTS``."""

    def __init__(self, sp: Spec, dim: int, optimizer="adagrad", lr=None, mode="as_built",
                 dtype=np.float64, perm=None, mutant=None, init=None, init_rows=None):
        from swiftsnails_amd.ops.optim import InitConfig

        assert optimizer in LR and mutant in (None,) + MUTANTS and mode in ("exact", "as_built")
        self.sp, self.D, self.opt = sp, dim, optimizer
        self.lr = LR[optimizer] if lr is None else lr
        self.mode = "exact" if sp.neg == "per_pair" else mode
        self.T, self.mutant = dtype, mutant
        self.ar = _Arith(dtype, perm)
        self.init = init or InitConfig("uniform", init_scale(dim), 0.0)
        self.init_rows = init_rows
        self.keys = np.empty(0, np.uint64)
        self.x, self.h = np.empty((0, dim), dtype), np.empty((0, dim), dtype)
        self.cdx = np.empty((0, dim))   # the steps' dx, summed (free-running SGD runs)
        self.ill, self.smax, self.losses, self.pairs = 0, 0.0, [], []
        self.flagged = self.elements = 0
        self.wide_coords = self.coords = 0

    def _insert(self, u):
        from swiftsnails_amd.ops.optim import init_reference

        pos = np.searchsorted(self.keys, u)
        hit = pos < len(self.keys)
        hit[hit] = self.keys[pos[hit]] == u[hit]
        new = u[~hit]
        if len(new):
            r = init_reference(self.init, new, self.D, 2 * self.D)
            if self.init_rows is not None:
                r[:, :self.D] = self.init_rows(new)
            keys = np.concatenate([self.keys, new])
            order = np.argsort(keys)
            self.keys = keys[order]
            self.x = np.concatenate([self.x, r[:, :self.D].astype(self.T)])[order]
            self.h = np.concatenate([self.h, r[:, self.D:].astype(self.T)])[order]
            self.cdx = np.concatenate([self.cdx, np.zeros((len(new), self.D))])[order]
            pos = np.searchsorted(self.keys, u)
        return pos

    def rebase(self, keys, x, h):
        self.keys = keys.copy()
        self.x, self.h = x.astype(self.T), h.astype(self.T)
        self.cdx = np.zeros(self.x.shape)

    def step(self, batches, pulled=None, observe=None, hull=False) -> Result:
        """One round on the ranks' batches ``[(keys [n_keys], meta), ...]``;
        ``pulled`` ([distinct keys, D]): the rows the gradient is computed
        from where they are not the state (a replayed pull-ahead round)."""
        pos = {}

        def rows_of(u):
            pos["p"] = self._insert(u)
            return (self.x[pos["p"]] if pulled is None else pulled).astype(np.float64)

        g = key_gradient(self.sp, batches, rows_of, self.mode, self.mutant, self.ar)
        p = pos["p"]
        x, h = self.x[p], self.h[p]
        x0, h0 = x.astype(np.float64), h.astype(np.float64)
        if observe is not None:    # settle the flagged elements from the state observed
            g.settle(observe(g.keys, x0, h0))
        if hull:                   # bf16 rows: the candidates' hull (Stepwise)
            g.eG = g.eG + g.hull
        self.nflip = getattr(self, "nflip", 0) + g.nflip
        G = g.G.astype(self.T)
        if self.mutant == "per_item_update":
            x, h = self._per_item(x, h, g)
        else:
            x, h = update(self.opt, self.lr, x, h, G, self.T)
        self.x[p], self.h[p] = x, h
        _, dh, ill = update_bound(self.opt, self.lr, h, G, g.eG)
        mid = update(self.opt, self.lr, x0, h0, g.G)[0]
        dx = np.maximum(np.abs(update(self.opt, self.lr, x0, h0, g.G + g.eG)[0] - mid),
                        np.abs(update(self.opt, self.lr, x0, h0, g.G - g.eG)[0] - mid))
        self.ill += int((ill & ~g.wide).any(1).sum())
        self.smax = max(self.smax, g.smax)
        self.losses.append(g.loss)
        self.pairs.append(g.pairs)
        self.flagged += g.flagged
        self.elements += g.elements
        self.wide_coords += int(g.wide.sum())
        self.coords += g.wide.size
        n = len(self.keys)
        tx, th = np.zeros((n, self.D)), np.zeros((n, self.D))
        tx[p], th[p] = dx, dh
        self.cdx[p] += dx
        touched, zero, wide = np.zeros(n, bool), np.zeros(n, bool), np.zeros((n, self.D), bool)
        touched[p], zero[p], wide[p] = True, g.zero, g.wide
        x64, h64 = self.x.astype(np.float64), self.h.astype(np.float64)
        return Result(self.keys.copy(), x64, h64, 1e-6 + 1e-4 * np.abs(x64) + tx,
                      1e-7 + 1e-4 * h64 + th, touched, zero, wide, g)

    def _per_item(self, x, h, g: Grad):
        """The mutant update: once per reduce item (32 occurrences) of a key."""
        Gocc = np.concatenate([o.G for o in g.occ])
        item = _occ_rank(g.inv) // CHUNK
        for c in range(int(item.max()) + 1):
            sel = item == c
            Gc = np.zeros_like(g.G)
            np.add.at(Gc, g.inv[sel], Gocc[sel])
            has = np.bincount(g.inv[sel], minlength=len(g.keys)) > 0
            xn, hn = update(self.opt, self.lr, x, h, Gc.astype(self.T), self.T)
            x, h = np.where(has[:, None], xn, x), np.where(has[:, None], hn, h)
        return x, h


def free_running_ratio(orc: W2VOracle, keys, x) -> float:
    """max |x - ref| / (1e-6 + 1e-4 |ref| + sum_t dx_t) of a model against a
    free-running (SGD) oracle over exactly its keys."""
    order = np.argsort(keys)
    assert np.array_equal(keys[order], orc.keys)
    ref = orc.x.astype(np.float64)
    return float((np.abs(x[order].astype(np.float64) - ref)
                  / (1e-6 + 1e-4 * np.abs(ref) + orc.cdx)).max())


def bf16_neighbour_ratio(x, ref, tol) -> float:
    """Compact bf16 rows, stored with stochastic rounding: every stored value
    must be one of the two bf16 neighbours of some value in ``ref +- tol``
    (the derived form of the rounding rule).  Returns the largest distance
    outside that range, in bf16 ulps of the reference (0: all inside)."""
    lo, hi = ref - tol, ref + tol
    # the bf16 number at or below lo / at or above hi
    dn = np.where(lo >= 0, bf16_trunc(lo), -_bf16_up(-lo))
    up = np.where(hi >= 0, _bf16_up(hi), -np.abs(bf16_trunc(hi)))
    out = np.maximum(dn - x, x - up)
    return float((np.maximum(out, 0) / np.maximum(bf16_ulp(ref), 2.0 ** -133)).max())


def _bf16_up(a):
    """The smallest bf16 number >= a, for a >= 0."""
    t = bf16_trunc(a)
    return np.where(t.astype(np.float32) == np.asarray(a, np.float32), t,
                    t + np.where(t != 0, bf16_ulp(np.where(t != 0, t, 1.0)), 2.0 ** -133))


class Stepwise:
    """Holds a model under test to the oracle one step at a time (as
    ``_fm_oracle.Stepwise``): before each step the oracle takes the model's
    own state, computes the step in fp64 with this step's bound, and the
    model's state after it must sit within ``tol`` for every key the batch
    touched; every other key, and every touched key whose gradient terms are
    all structurally zero, must be bit-identical."""

    def __init__(self, sp: Spec, dim, optimizer, lr=None, mode="as_built", init=None,
                 init_rows=None, strict=True, bf16_rows=False):
        self.orc = W2VOracle(sp, dim, optimizer, lr, mode, init=init, init_rows=init_rows)
        self.bf16_rows = bf16_rows   # stored values: a bf16 neighbour of ref +- tol
        self.strict, self.broken = strict, 0   # not strict: bit-identity misses are counted
        self.keys = np.empty(0, np.uint64)
        self.x = self.h = np.empty((0, dim))
        self.rx = self.rh = self.out = 0.0
        self.rx_plain = self.rh_plain = 0.0   # over the coordinates no flagged element feeds

    @property
    def ill(self):
        return self.orc.ill

    def step(self, batches, keys, x, h=None, pulled=None):
        o = self.orc
        o.rebase(self.keys, self.x, self.h)
        order = np.argsort(keys)
        keys, x = keys[order], x[order].astype(np.float64)
        h = h[order].astype(np.float64) if h is not None else np.zeros_like(x)

        def observe(u, x0, h0):
            """The gradient the model's step implies, per key of the batch (to
            well below a flip's size: AdaGrad's state moves by exactly G^2)."""
            pos = np.searchsorted(keys, u).clip(max=len(keys) - 1)
            assert np.array_equal(keys[pos], u), "a key of the batch is not in the table"
            if o.opt == "adagrad":
                return np.sign(x0 - x[pos]) * np.sqrt(np.maximum(h[pos] - h0, 0))
            return (x0 - x[pos]) / o.lr

        # compact bf16 rows cannot be decoded (their rounding is 2^-8 relative); there the
        # candidates' hull is the exact candidate set (module docstring)
        r = o.step(batches, pulled=pulled, observe=None if self.bf16_rows else observe,
                   hull=self.bf16_rows)
        assert len(keys) == len(r.keys) and np.array_equal(keys, r.keys), (len(keys), len(r.keys))
        # untouched keys, and structurally zero gradients (the oracle's own
        # step of G = 0 is x - lr 0 = x, exactly): bit for bit
        same = ~r.touched | r.zero
        bad = int(((x[same] != r.x[same]) | (h[same] != r.h[same])).any(1).sum())
        assert not (bad and self.strict), (bad, int(same.sum()))
        self.broken += bad
        if self.bf16_rows:
            bx, bh = bf16_neighbour_ratio(x, r.x, r.tol_x), bf16_neighbour_ratio(h, r.h, r.tol_h)
            self.rx, self.rh = max(self.rx, bx), max(self.rh, bh)
            self.keys, self.x, self.h, self.last = keys, x, h, r
            return bx, bh
        rx, rh = np.abs(x - r.x) / r.tol_x, np.abs(h - r.h) / r.tol_h
        self.rx, self.rh = max(self.rx, float(rx.max())), max(self.rh, float(rh.max()))
        plain = ~r.wide
        if plain.any():
            self.rx_plain = max(self.rx_plain, float(rx[plain].max()))
            self.rh_plain = max(self.rh_plain, float(rh[plain].max()))
        self.out = max(self.out, float(((rx > 1) | (rh > 1)).any(1).mean()))
        self.keys, self.x, self.h, self.last = keys, x, h, r
        return float(rx.max()), float(rh.max())


# --------------------------------------------------------------------- data
def _word(i):
    """A quarter of the word ids carry bits 32..39 (12-byte dedup records)."""
    i = np.asarray(i, np.uint64)
    hi = (i % np.uint64(7) + np.uint64(1)) << np.uint64(32)
    return np.where(i % np.uint64(4) == 0, i | hi, i)


PLANT0 = 2_000_000          # planted word ids: outside every drawn vocabulary
W_TAIL, W_C33, W_HOT, W_BOTH = PLANT0 + 900, PLANT0 + 33, PLANT0 + HOT, PLANT0 + 64


@dataclass
class Data:
    name: str
    sp: Spec
    keys: np.ndarray     # [STEPS, n_keys] uint64
    meta: np.ndarray     # [STEPS, R] int32 (window layout) or None
    plan: list           # per step {count: output key}
    tail_pos: tuple = ()  # run positions of the tail-zone key (window layout)
    lone: int = -1        # run position of the one-token sentence (a center without pairs)

    def batch(self, t):
        return self.keys[t % STEPS], (self.meta[t % STEPS] if self.meta is not None else None)


def plan_counts(cap: int, step: int):
    """The planted occurrence counts of a step that fit 90 % of ``cap`` output
    slots: all of them, or alternating (module docstring)."""
    full = COUNTS + (HOT,)
    if sum(full) <= 0.9 * cap:
        return full[::-1]
    out = []
    for c in (COUNTS[:5] + (HOT,) if step % 2 else COUNTS):   # the small ones first
        if sum(out) + c <= 0.9 * cap:
            out.append(c)
    return tuple(out[::-1])                                    # planted largest first


def tail_positions(sp: Spec):
    """The run positions at the edges of the tail zone ``q >= 64, q % 64 <
    2W`` (63, 64, 64 + 2W - 1, 64 + 2W) and of the last partial tile's."""
    W, out = sp.W, []
    if sp.tiles > 1:
        out += [63, 64, 64 + 2 * W - 1, 64 + 2 * W]
        t0 = TILE * (sp.tiles - 1)
        if sp.B % TILE and sp.tiles > 2:
            out += [t0, t0 + 2 * W - 1, t0 + 2 * W]
    return tuple(sorted({q for q in out if q < sp.R}))


@functools.lru_cache(maxsize=None)
def dataset(name: str, sp: Spec, seed: int = 0, vocab: int = 3000) -> Data:
    rng = np.random.default_rng([seed, sp.B, sp.W, sp.K, sp.layout == "window",
                                 sp.neg == "shared"])
    B, W, R, n = sp.B, sp.W, sp.R, sp.n_keys
    window = sp.layout == "window"
    keys = np.zeros((STEPS, n), np.uint64)
    meta = np.full((STEPS, R), -1, np.int32) if window else None
    plans = []
    tails = tail_positions(sp) if window else ()
    lone = W + 20 if window and B > 24 else -1
    draw = lambda size: _word(rng.zipf(1.3, size) % vocab + 1)  # noqa: E731
    for t in range(STEPS):
        ctx0, neg0 = B, B + sp.n_ctx
        keys[t, ctx0:neg0] = draw(sp.n_ctx) | OUT
        if sp.neg == "per_pair":  # most negatives once, a Zipf head hundreds of times
            head = rng.random(sp.n_neg) < 0.3
            keys[t, neg0:] = np.where(head, _word(rng.zipf(1.3, sp.n_neg) % 50 + 1),
                                      _word(rng.integers(10_000, 1_000_000, sp.n_neg))) | OUT
        else:
            keys[t, neg0:] = draw(sp.n_neg) | OUT
        reserved = set()
        if window:
            # sentences: random boundaries, boundaries exactly at the tile
            # boundaries of the centers (run positions W + 64 k), a one-token
            # sentence; reduced windows in [1, W], some 1, some W; masked ones
            start = rng.random(R) < 0.08
            start[[q for q in (W + TILE, W + 2 * TILE) if q < R]] = True
            if lone >= 0:
                start[[lone, lone + 1]] = True
            tag = np.cumsum(start) + 16 * t
            b = rng.integers(1, W + 1, R)
            b[rng.random(R) < 0.15] = 1
            b[rng.random(R) < 0.15] = W
            m = ((tag << 4) | b).astype(np.int32)
            dead = rng.random(R) < 0.06
            dead[list(tails)] = False
            if lone >= 0:
                dead[lone] = False
            m[dead] = -1
            meta[t] = m
            for q in tails:
                keys[t, ctx0 + q] = _word(W_TAIL) | OUT
                reserved.add(ctx0 + q)
            if lone >= 0:
                reserved.add(ctx0 + lone)
        free_ctx = [i for i in range(ctx0, neg0) if i not in reserved]
        plan = {}
        counts = plan_counts(sp.n_ctx + sp.n_neg, t)
        free_neg = list(range(neg0, n))
        for c in sorted(counts, key=lambda c: (c != 33, -c)):   # the centers' key first
            key = _word(PLANT0 + c) | OUT
            plan[c] = int(key)
            if c == HOT:   # contiguous: the head of the negatives, then run positions
                # (as many run positions as the other counts leave free, at least
                # a whole tile's 64 negatives)
                take = free_neg[:min(len(free_neg), max(64, c - max(0, len(free_ctx) - 110)))]
                free_neg = free_neg[len(take):]
                rest = c - len(take)
                take += free_ctx[:rest]
                free_ctx = free_ctx[rest:]
            elif c == 33 and window:   # all 33 among the centers' positions: a center 33 times
                cen = [i for i in free_ctx if W <= i - ctx0 < W + B]
                take = list(rng.choice(cen, 33, replace=False))
                free_ctx = [i for i in free_ctx if i not in set(take)]
            else:
                nctx = min(len(free_ctx), max(1, c // 6) if c == 64 else
                           int(rng.integers(0, c + 1)))
                nctx = max(min(nctx, len(free_ctx) // 4), c - len(free_neg))
                ci = list(rng.choice(len(free_ctx), nctx, replace=False)) if nctx else []
                ni = list(rng.choice(len(free_neg), c - nctx, replace=False)) if c > nctx else []
                take = [free_ctx[i] for i in ci] + [free_neg[i] for i in ni]
                free_ctx = [x for j, x in enumerate(free_ctx) if j not in set(ci)]
                free_neg = [x for j, x in enumerate(free_neg) if j not in set(ni)]
            keys[t, take] = key
        if sp.neg == "per_pair" and window:   # a negative equal to a run position's key
            keys[t, free_neg[0]] = keys[t, free_ctx[0]]
        if window:
            keys[t, :B] = keys[t, ctx0 + W:ctx0 + W + B] & ~OUT
        else:
            keys[t, :B] = draw(B)
            keys[t, rng.choice(B, 33, replace=False)] = _word(W_C33)
        plans.append(plan)
    return Data(name, sp, keys, meta, plans, tails, lone)


WIN = Spec("window", "shared", 200, 5)
WIN_EDGE = {"b64": Spec("window", "shared", 64, 5), "b65": Spec("window", "shared", 65, 5),
            "b128": Spec("window", "shared", 128, 5), "w1": Spec("window", "shared", 100, 1),
            "w15": Spec("window", "shared", 100, 15)}
PAIRS = {"b128w2": Spec("pairs", "shared", 128, 2), "b100w5": Spec("pairs", "shared", 100, 5)}
PP = {"w2k1": Spec("window", "per_pair", 70, 2, 1), "w5k5": Spec("window", "per_pair", 200, 5, 5),
      "w5k6": Spec("window", "per_pair", 70, 5, 6), "w3k11": Spec("window", "per_pair", 200, 3, 11),
      "w15k16": Spec("window", "per_pair", 70, 15, 16)}


def cases() -> dict:
    """name -> Spec of every data set."""
    out = {"w2v_win": WIN}
    out.update({f"w2v_win_edge/{k}": v for k, v in WIN_EDGE.items()})
    out.update({f"w2v_pairs/{k}": v for k, v in PAIRS.items()})
    out.update({f"w2v_pp/{k}": v for k, v in PP.items()})
    return out


def data(name: str, rank: int = 0) -> Data:
    return dataset(name, cases()[name], seed=rank)


def batches(name: str, world: int = 1, steps: int = STEPS):
    """Per step the ranks' batches ``[(keys, meta), ...]``: a synchronous round."""
    ds = [data(name, r) for r in range(world)]
    return [[d.batch(t) for d in ds] for t in range(steps)]


def run(name, dim, optimizer="adagrad", world=1, steps=STEPS, **kw) -> W2VOracle:
    orc = W2VOracle(cases()[name], dim, optimizer, **kw)
    for b in batches(name, world, steps):
        orc.step(b)
    return orc


def stepwise(name, dim, optimizer="adagrad", world=1, mode="as_built", steps=STEPS,
             **kw) -> Stepwise:
    """A free-running model (the fp32 emulation, or a mutant) held to the
    oracle step by step."""
    sp = cases()[name]
    model = W2VOracle(sp, dim, optimizer, mode=mode, **kw)
    sw = Stepwise(sp, dim, optimizer, mode=mode, strict=kw.get("mutant") is None)
    for b in batches(name, world, steps):
        model.step(b)
        sw.step(b, model.keys, model.x, model.h)
    sw.model = model
    return sw


# ------------------------------------------------------------ planted source
class PlantedW2V(W2VLayout):
    """A ``Word2VecWorker`` data source that copies a data set's precomputed
    key and meta arrays into the worker's buffers (on the given stream), step
    t modulo ``STEPS``.  Not graph-capturable."""

    graph_capturable = False

    def __init__(self, d: Data, device):
        import torch

        sp = d.sp
        self.batch_size, self.window, self.negatives = sp.B, sp.W, sp.K
        self.mode, self.neg_mode = sp.layout, sp.neg
        self._check_mode()
        assert self.n_keys == sp.n_keys and self.n_neg == sp.n_neg
        self.d_keys = torch.from_numpy(d.keys.view(np.int64)).to(device)
        self.d_meta = torch.from_numpy(d.meta).to(device) if d.meta is not None else None
        torch.cuda.synchronize(device)

    def generate(self, step, rank, world, keys, stream=None, step_dev=0, step_delta=0, meta=None):
        import torch

        if step_dev:
            raise RuntimeError("planted batches cannot be replayed from a graph")
        if self.mode == "window" and (meta is None or meta.numel() < self.run_len):
            raise ValueError("window mode: generate() needs a meta buffer of run_len int32")
        st = stream
        if isinstance(st, int):
            st = torch.cuda.ExternalStream(st)
        t = step % STEPS
        with torch.cuda.stream(st if st is not None else torch.cuda.current_stream()):
            keys[:self.n_keys].copy_(self.d_keys[t], non_blocking=True)
            if self.mode == "window":
                meta[:self.run_len].copy_(self.d_meta[t], non_blocking=True)
