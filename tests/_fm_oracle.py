"""A high-precision factorization-machine reference with an error bound, and its data.

Built like ``_lr_oracle.py`` and sharing what fits (``Dataset`` and its
libsvm writer, ``EMPTY``, ``U32``, ``U_G`` with its derivation).  Nothing here
comes from the engine except ``init_reference``, the host mirror of the
key-seeded initialiser.

The initialiser.  FM rows start from the *normal* initialiser, whose host
mirror is not bit-exact with the device (``__logf`` / ``__cosf`` there,
NumPy's here).  The GPU tests start the oracle from rows read back: new keys
take the rows a scratch table with the same ``InitConfig`` returns for them
(``FMOracle(init_rows=...)``; the initialiser is a function of key and
column alone).  ``test_gpu_fm_paths_oracle.py::test_device_init_within_the_
relative_term`` also measures the host mirror against the device once, every
key and 17 columns: at most 1.9e-8 apart, 0.015 of ``1e-6 + 1e-4 |x|``.  The
CPU tests and the free-running references start from the host mirror.

Data sets (``dataset(name)``; B = 4096, 8 steps = 32768 rows, libsvm text)
-------------------------------------------------------------------------
Binary features (``label idx idx ...``).  Rows hold 3..F entries, a few rows
none; short rows are padded with the EMPTY key.  A quarter of the distinct
drawn indices carry bits at or above 2^32 (a function of the index).  Labels
are Bernoulli draws of a planted linear model.

* ``fm_spread`` (F = 13).  LR's ``zipf(1.3)`` puts a quarter of all
  occurrences on one key; the head here is moderate: ranks follow the
  Zipf-Mandelbrot law ``P(r) ~ 1 / (r + 50)`` over 2e6 ranks (the hottest
  drawn key has 60-70 occurrences per batch, ~140 keys have more than 16,
  18k are singletons, 118538 distinct keys in all), mapped to indices as LR
  does (``r * 7919 % 2_000_003 + 1``).  Planted on top, in every batch: key
  ``P16`` with exactly 16 occurrences and ``P17`` with exactly 17 (the
  ``kFmLong`` boundary of the sorted merge: a thread per list up to 16, a
  wave per longer list), and ``P300`` with 300 (the wave-per-list path, a
  tail of 300 mod 64 = 44), 20 of them as pairs inside ten samples (a key
  repeated within a sample; the drawn head adds 20-36 such pairs a batch).
* ``fm_narrow`` (F = 6): the same generator at six fields.  The forward's
  lane-group width ``1 << (F - 1).bit_length()`` = 8 is then below K = 16, so
  ``FMWorker`` itself chooses the row-atomic fallback at ``dim`` 17.
* ``fm_hot`` (F = 13): the same with key ``HOT`` planted 11000 times in every
  batch (a third of its occurrences, several in one sample): its dedup
  bucket holds more than ``kFmOcc`` = 10240 occurrences and goes to the
  overflow list and the LDS-atomic merge.  SGD runs at lr = 1e-4 (the hot
  key's ``G_w`` is a sum of 11000 terms, ~1e3: a step then moves its w by
  ~0.1); the oracle records max |z| = 0.96, below 20.  With AdaGrad the
  oracle alone reports no ill-conditioned key-step either (K = 8 and 16, max
  |z| 1.4), so that case runs too.

The model (``FMOracle``), rows ``[w | v_1..v_K]``, K in {1, 4, 8, 16}
--------------------------------------------------------------------
Every non-EMPTY occurrence (s, j) counts as a feature: a key that occurs
twice in a sample counts twice.  Per sample s and factor f

    S_sf  = sum_j v[k_sj, f]
    z_s   = sum_j w[k_sj] + 1/2 sum_f [S_sf^2 - sum_j v[k_sj, f]^2]
    g_s   = sigmoid(z_s) - y_s
    loss_s = max(z_s, 0) + log1p(exp(-|z_s|)) - y_s z_s

and per key k with occurrences O, per coordinate,

    G_w = sum_O g_s            G_f = sum_O g_s (S_sf - v_kf)
    adagrad:  h += G^2 ;  x -= lr G / sqrt(h + eps)        (lr 0.05, eps 1e-8)
    sgd:      x -= lr G                                    (lr 1e-3)

once per key and step; a key seen for the first time starts from the
initialiser (normal, scale 0.01; h = 0), as ``fm_table_args`` sets.

The bound of one step (``grad_bound``)
--------------------------------------
u = 2^-24 is the fp32 unit round-off and ``U_G`` = 2^-21 the relative
accuracy of one ``g_s`` from ``__expf`` (``_lr_oracle.py`` derives it).  Two
things FM needs beyond LR's bound, both from the arithmetic alone:

* the absolute accuracy of ``g_s`` is ``U_A`` = 1.5 u, not u: in ``p = 1 /
  (1 + e)`` the sum ``1 + e`` lies in [1, 2), where fp32 numbers are 2^-23
  apart, so rounding it moves p (<= 1) by up to 2^-24, and the division
  rounds p by 2^-25 more; ``p - y`` is exact.  Where |g| is small (|z| of 4
  and more, label matched) nothing else covers it: the fp32 NumPy evaluation
  of one gradient at the kernel tests' sizes (rows of scale 0.1, |z| up to
  16) misses a bound with u in its place, and without dz below, by up to
  1.45; with both it stays at 0.84 and below
  (``test_fm_oracle_cpu.py::test_key_gradient_fp32_floor``; the training data
  sets have |z| below 1.4 and are not affected).
* z's own fp32 summation: g moves by p (1 - p) dz = |g| (1 - |g|) dz (y is 0
  or 1), a relative amount.  For the form the kernels compute (per
  occurrence ``t_j = w_j - sq_j / 2`` with ``sq_j = sum_f v_jf^2``, the F
  ``t_j`` summed in any order, then ``+ S_f^2 / 2`` factor by factor), to
  first order in u, with T1 = sum_j |t_j|:

      dz_s = u [ F T1 + K/2 sum_j sq_j + sum_f (|S_f| (F - 1) sum_j |v_jf| + S_f^2)
                 + K (T1 + 1/2 sum_f S_f^2) ]

  (F T1: the any-order sum and each t_j's own rounding; K/2 sq: the K
  products and additions inside sq_j; the sum over f: S_f's rounding through
  the square, and the square's and the halving's own; the last: K additions
  to the running z.)

For key k, occurrences O, with r_s = |g_s| (U_G + (1 - |g_s|) dz_s) and
A_w = sum_O |g_s|:

    eG_w = sum_O r_s + U_A |O| + |O| u A_w

(each term's relative accuracy; each term's absolute accuracy; any fp32
summation order of |O| terms).  The v coordinates are bounded over the
factored form the merge kernels use, ``sum_O gss_sf - v_kf sum_O g_s`` with
``gss_sf = fl(g_s S_sf)`` and ``S_sf`` an fp32 sum of the sample's F rows in
any order:

    A_f   = sum_O |g_s S_sf| + |v_kf| sum_O |g_s|
    eS_sf = (F - 1) u sum_j |v[k_sj, f]|
    eG_f  = sum_O r_s (|S_sf| + |v_kf|) + U_A sum_O max(1, |S_sf| + |v_kf|)
            + |O| u A_f + sum_O |g_s| eS_sf

``r_s (|S| + |v|)``: the relative accuracy of g_s in both products (the two
products' own roundings, u each, sit inside the factor 2 spared in ``U_G``).
The second term: the absolute accuracy of g_s reaches the term through the
factors S_sf and v_kf, and is never taken below the w coordinate's.
``|O| u A_f``: any summation order of both sums, the product ``v_kf G0``
carrying G0's own ``|O| u A_w``, and the final subtraction.  The last term:
S_sf's rounding times |g_s|.  The row-atomic fallback forms ``g_s (S_sf -
v_kf)`` per occurrence, whose every error term is below the factored form's
(|S - v| <= |S| + |v|), so one bound serves all kernels.

    adagrad:  dx_t = lr eG / sqrt(h_after + eps),  dh_t = 2 |G| eG + eG^2
    sgd:      dx_t = lr eG
    tol_x = 1e-6 + 1e-4 |x| + sum_t dx_t
    tol_h = 1e-7 + 1e-4  h  + sum_t dh_t

per key and coordinate (the relative 1e-4 holds ``__frsqrt_rn`` and the
update's own roundings, as for LR).  Nothing is fitted to kernel output.

No key is excused: a key-step is *ill-conditioned* when, for any coordinate,
``eG > 0.1 sqrt(h_after + eps)`` (AdaGrad).  No data set has one for any K
(``Result.ill == 0``, asserted from the oracle alone before anything is
compared with it, and again on the trajectory of the model under test).

Why AdaGrad is held step by step (``Stepwise``)
-----------------------------------------------
The sum over t above is a bound carried beside a free-running state, as for
LR.  For FM under AdaGrad it does not describe even the reference's own fp32
evaluation.  Measured on ``fm_spread``, eight free-running steps, three
permutations, max |fp32 - fp64| / tol (x, h) and the coordinates outside:

    K      direct  x      h     outside          factored  x      h     outside
    1              213    491   536 of 237076              415    887   724
    4              16.5   25.5  716 of 592690              11.5   66.8  1039
    8              9.4    19.4  324 of 1066842             18.5   22.5  352
    16             51.9   31.9  1247 of 2015146            42.3   54.9  1259

The steps themselves are fine (below).  A v coordinate's gradient ``g (S_f -
v_f)`` is small by chance where LR's ``g x`` never is; such a coordinate's
first AdaGrad step is ``-lr G / sqrt(G^2 + eps)``, which between |G| = 0 and
1e-4 turns what the *other* rows of its sample carry into 500 times as much
(lr / sqrt(eps)): a few coordinates in a hundred thousand amplify their
neighbours' legitimate 1e-7 to 1e-4, and the keys sharing samples with them
inherit that in the next step.  No rounding of the step itself is involved,
so no per-step term, and no seed, removes it; propagating the carried bound
through the forward to first order, worst case, gives tolerances of 1e3 and
more within eight steps, which holds nothing.  The rule for ill-conditioned
key-steps does not see it (``eG`` is 1e-7, ``0.1 sqrt(eps)`` is 1e-5) and is
not changed.

So a model under test is held to the oracle one step at a time: ``Stepwise``
takes the model's own state before each step (exactly), computes the step in
fp64 with this step's bound ``tol = 1e-6 + 1e-4 |x| + dx_t`` (h alike), and
the model's state after the step must sit within it for every key and
coordinate the batch touched and be bit-identical for every other; the
model's state is then the next step's start.  Every step of every key is
checked, no error is carried, and nothing accumulates that a bound would
have to cover.  SGD has no denominator: its carried bound holds, and SGD
cases are held to the free-running reference as well.

Measured on the CPU (``test_fm_oracle_cpu.py``)
-----------------------------------------------
fp32 noise floor, step by step, three permutations of every sum, max
|fp32 - fp64| / tol over every key and coordinate (x: parameters, h: state):

    fm_spread  adagrad  K      direct  x      h        factored  x      h
                        1              0.044  0.034              0.051  0.038
                        4              0.078  0.029              0.078  0.029
                        8              0.049  0.029              0.098  0.029
                        16             0.060  0.034              0.068  0.034
    fm_narrow  adagrad  16             0.088  0.029              0.088  0.030
    fm_hot     adagrad  8              0.066  0.036              0.066  0.036
    fm_spread  sgd      8              0.002  -                  0.002  -
    fm_hot     sgd      8              0.001  -                  0.001  -

Free-running SGD, eight steps against the carried bound: 0.002 (``fm_spread``)
and 0.003 (``fm_hot``) in both forms.  Max |z|: 1.2-1.4 with AdaGrad, 0.41
with SGD, 0.96 on ``fm_hot`` with SGD; median tol_x 6.4e-6 at median |x|
5.0e-2 (AdaGrad), 1.7e-6 at 6.7e-3 (SGD).

Planted mutants on ``fm_spread``, AdaGrad, step by step: max ratio (x, h) and
the share of keys outside, K = 8 (K = 1, 4, 16 alike; the smallest max ratio
of all 32 runs is 9.6e3); none is weakly detected (below 2):

    v_not_subtracted   x 7.3e4  h 1.2e6   99.9 %
    v_once_per_key     x 8.5e4  h 6.4e5   99.9 %
    no_self_term       x 3.1e4  h 1.3e5   100 %
    dup_once           x 5.7e4  h 8.9e4   1.6 %
    wave_tail          x 3.6e4  h 1.4e4   0.7 %
    gss_stride         x 8.9e4  h 3.2e6   100 %
    per_occurrence     x 1.2e5  h 2.2e7   14.1 %
    h_shifted          x 0      h 7.7e8   100 %

(``h_shifted``: x 0 because each step starts from the mutant's own h.)
On the MI355X the engine sits at the same floor: at most 0.081 (x) and 0.041
(h) over every path of ``test_gpu_fm_paths_oracle.py``.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from _lr_oracle import B, EMPTY, ROWS, STEPS, U32, U_G, Dataset, update, update_bound

F = {"fm_spread": 13, "fm_hot": 13, "fm_narrow": 6}
KS = (1, 4, 8, 16)
LR = {"adagrad": 0.05, "sgd": 1e-3}
HOT_SGD_LR = 1e-4
U_A = 1.5 * U32  # absolute accuracy of one g_s (module docstring)
INIT_SCALE, EPS = 0.01, 1e-8
SEEDS = {"fm_spread": 11, "fm_hot": 12, "fm_narrow": 13}
P16, P17, P300, HOT = (np.uint64(2_100_000 + i) for i in (16, 17, 300, 1))
N_HOT, KFM_LONG, KFM_OCC = 11000, 16, 10240
MANDELBROT_Q, RANKS = 50.0, 2_000_000


# ------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def dataset(name: str) -> Dataset:
    rng = np.random.default_rng(SEEDS[name])
    nf = F[name]
    n = rng.integers(3, nf + 1, ROWS)
    n[rng.choice(ROWS, 7, replace=False)] = 0  # a few empty rows
    mask = np.arange(nf)[None, :] < n[:, None]
    # Zipf-Mandelbrot ranks: the inverse CDF of the density 1 / (x + q) on [0, RANKS)
    x = MANDELBROT_Q * ((1.0 + RANKS / MANDELBROT_Q) ** rng.random((ROWS, nf)) - 1.0)
    r = np.minimum(x.astype(np.int64) + 1, RANKS)
    idx = (r * 7919 % 2_000_003 + 1).astype(np.uint64)
    idx = np.where(idx % np.uint64(4) == 0,  # a quarter of the indices above 2^32
                   idx | ((idx % np.uint64(7) + np.uint64(1)) << np.uint64(32)), idx)
    keys = np.where(mask, idx, EMPTY)
    for t in range(STEPS):  # the planted keys, batch by batch
        rows = np.arange(t * B, (t + 1) * B)
        pairs = rows[n[rows] >= 2][:10]          # P300 twice in each of ten samples
        keys[pairs, 0] = keys[pairs, 1] = P300
        free = np.setdiff1d(rows, pairs)
        rr, cc = np.nonzero(mask[free])
        order = rng.permutation(len(rr))
        plan = [(P16, 16), (P17, 17), (P300, 280)] + ([(HOT, N_HOT)] if name == "fm_hot" else [])
        at = 0
        for key, cnt in plan:
            sel = order[at:at + cnt]
            keys[free[rr[sel]], cc[sel]] = key
            at += cnt
    # labels from a planted linear model over the distinct keys (planted keys neutral)
    u, inv = np.unique(keys, return_inverse=True)
    truth = rng.normal(0.0, 1.0, len(u))
    truth[np.isin(u, [P16, P17, P300, HOT, EMPTY])] = 0.0
    z = (truth[inv.reshape(ROWS, nf)] * mask).sum(1) - 0.5
    y = (rng.random(ROWS) < 1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    lines = [(" ".join([str(int(y[i]))] + [str(int(k)) for k in keys[i, :n[i]]]) + "\n").encode()
             for i in range(ROWS)]
    return Dataset(name, keys, mask.astype(np.float32), y, lines)


# ------------------------------------------------------------------ model
MUTANTS = ("v_not_subtracted", "v_once_per_key", "no_self_term", "dup_once", "wave_tail",
           "gss_stride", "per_occurrence", "h_shifted")


@dataclass
class Result:
    keys: np.ndarray    # sorted, distinct
    x: np.ndarray       # [n, 1 + K] parameters
    h: np.ndarray       # [n, 1 + K] AdaGrad state (zeros with sgd)
    tol_x: np.ndarray
    tol_h: np.ndarray
    losses: list        # per step: per-sample losses (fp64)
    ill: int            # ill-conditioned key-steps
    zmax: float

    def mean_losses(self, world: int = 1) -> np.ndarray:
        """[steps, world]: each rank's mean loss (the batch is the ranks'
        batches concatenated)."""
        return np.array([l.reshape(world, -1).mean(1) for l in self.losses])


def _occ_rank(inv: np.ndarray):
    """Number of each occurrence within its key's list (in occurrence order)."""
    order = np.argsort(inv, kind="stable")
    k = inv[order]
    rank = np.empty(len(inv), np.int64)
    rank[order] = np.arange(len(k)) - np.searchsorted(k, k)
    return rank


def grad_bound(X, s, inv, R, g, nu):
    """``eG`` [nu, 1 + K] of the module docstring, in fp64: ``X`` [B, F, 1 + K]
    the occurrence rows (zero where there is none), ``s`` / ``inv`` each
    occurrence's sample / unique row, ``R`` [nu, 1 + K] the unique rows, ``g``
    [B] the samples' gradient factors."""
    X, R, g = X.astype(np.float64), R.astype(np.float64), g.astype(np.float64)
    nf, K = X.shape[1], X.shape[2] - 1
    V = X[..., 1:]
    S, absV, sq = V.sum(1), np.abs(V).sum(1), (V * V).sum(2)           # [B, K], [B, K], [B, F]
    T1 = np.abs(X[..., 0] - 0.5 * sq).sum(1)
    eS = (nf - 1) * U32 * absV
    dz = (nf * T1 + 0.5 * K * sq.sum(1) + (np.abs(S) * eS / U32 + S * S).sum(1)
          + K * (T1 + 0.5 * (S * S).sum(1))) * U32
    ag = np.abs(g)
    rel = (ag * (U_G + (1 - ag) * dz))[s]       # per occurrence: |g_s| (U_G + (1 - |g_s|) dz_s)
    cnt = np.bincount(inv, minlength=nu)
    Aw = np.bincount(inv, ag[s], minlength=nu)
    eG = np.empty((nu, 1 + K))
    eG[:, 0] = np.bincount(inv, rel, minlength=nu) + U_A * cnt + cnt * U32 * Aw
    for f in range(K):
        Sf, vf = np.abs(S[s, f]), np.abs(R[inv, 1 + f])
        Af = np.bincount(inv, ag[s] * Sf, minlength=nu) + np.abs(R[:, 1 + f]) * Aw
        eG[:, 1 + f] = (np.bincount(inv, rel * (Sf + vf), minlength=nu)
                        + U_A * np.bincount(inv, np.maximum(1.0, Sf + vf), minlength=nu)
                        + cnt * U32 * Af + np.bincount(inv, ag[s] * eS[s, f], minlength=nu))
    return eG


class FMOracle:
    """The FM over a sorted key set.  ``dtype`` float64 is the reference;
    float32 with ``perm`` (a seed) evaluates the same model in fp32 with every
    sum's order permuted, in the ``direct`` form (terms ``g (S - v)``) or the
    kernels' ``factored`` form (fp32 ``S``, fp32 ``gss = g S``, then ``sum gss
    - v sum g``).  ``mutant`` plants one of ``MUTANTS``: each is a way an FM
    kernel can be subtly wrong."""

    def __init__(self, K: int, optimizer: str = "adagrad", lr: float | None = None,
                 dtype=np.float64, perm: int | None = None, form: str = "direct",
                 mutant: str | None = None, init_rows=None):
        from swiftsnails_amd.ops.optim import InitConfig

        assert K in KS and optimizer in LR and mutant in (None,) + MUTANTS
        assert form in ("direct", "factored")
        self.K, self.D = K, 1 + K
        self.opt, self.lr = optimizer, LR[optimizer] if lr is None else lr
        self.T, self.form, self.mutant = dtype, form, mutant
        self.rng = np.random.default_rng(perm) if perm is not None else None
        self.init = InitConfig("normal", INIT_SCALE, 0.0)
        self.init_rows = init_rows  # keys -> [n, 1 + K] initial parameters (else the host mirror)
        self.keys = np.empty(0, np.uint64)
        self.x, self.h = np.empty((0, self.D), dtype), np.empty((0, self.D), dtype)
        self.dx, self.dh = np.empty((0, self.D)), np.empty((0, self.D))
        self.ill, self.zmax, self.losses = 0, 0.0, []

    def _insert(self, u: np.ndarray) -> np.ndarray:
        """Positions of the sorted distinct keys ``u``; new ones inserted with
        their initial row."""
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
            z = np.zeros((len(new), self.D))
            self.keys = keys[order]
            self.x = np.concatenate([self.x, r[:, :self.D].astype(self.T)])[order]
            self.h = np.concatenate([self.h, r[:, self.D:].astype(self.T)])[order]
            self.dx = np.concatenate([self.dx, z])[order]
            self.dh = np.concatenate([self.dh, z])[order]
            pos = np.searchsorted(self.keys, u)
        return pos

    def rebase(self, keys: np.ndarray, x: np.ndarray, h: np.ndarray) -> None:
        """Take (keys sorted and distinct, x, h) as the state, exactly."""
        self.keys = keys.copy()
        self.x, self.h = x.astype(self.T), h.astype(self.T)
        self.dx, self.dh = np.zeros(self.x.shape), np.zeros(self.x.shape)

    def _sum(self, inv, term, nu):
        """sum of ``term`` per key: fp64 exactly enough; fp32 sequentially in a
        permuted order."""
        if self.rng is None:
            return np.bincount(inv, term, minlength=nu).astype(self.T)
        order = self.rng.permutation(len(term))
        G = np.zeros(nu, self.T)
        np.add.at(G, inv[order], term[order])
        return G

    def step(self, keys: np.ndarray, y: np.ndarray, pulled: np.ndarray | None = None):
        """One round on a batch ``keys`` [B, F] / ``y`` [B].  ``pulled``
        ([distinct keys of the batch, sorted; 1 + K]): the rows the gradient
        is computed from, where they are not the state (a replayed pull-ahead
        round); the update is applied to the state either way."""
        T, mut, K, D = self.T, self.mutant, self.K, self.D
        nb, nf = keys.shape
        mask = keys != EMPTY
        if mut == "dup_once":  # a key repeated in a sample counts once
            srt = np.sort(np.where(mask, keys, EMPTY), axis=1)
            keys = np.concatenate([srt[:, :1], np.where(srt[:, 1:] == srt[:, :-1], EMPTY,
                                                        srt[:, 1:])], axis=1)
            mask = keys != EMPTY
        s = np.nonzero(mask)[0]                    # sample of each occurrence
        u, inv = np.unique(keys[mask], return_inverse=True)
        nu, cnt = len(u), np.bincount(inv, minlength=len(u))
        pos = self._insert(u)
        R = (self.x[pos] if pulled is None else pulled.astype(T))
        X = np.zeros((nb, nf, D), T)
        X[mask] = R[inv]
        # forward (fp32: the fields in a permuted order)
        cols = self.rng.permutation(nf) if self.rng is not None else range(nf)
        S, zw = np.zeros((nb, K), T), np.zeros(nb, T)
        if self.form == "factored":  # per row w - sq / 2, summed; then + S^2 / 2 per factor
            for j in cols:
                sq = np.zeros(nb, T)
                for f in range(K):
                    sq = sq + X[:, j, 1 + f] * X[:, j, 1 + f]
                zw = zw + (X[:, j, 0] - T(0.5) * sq)
                S = S + X[:, j, 1:]
            z = zw
            for f in range(K):
                z = z + T(0.5) * S[:, f] * S[:, f]
        else:
            sq = np.zeros((nb, K), T)
            for j in cols:
                zw = zw + X[:, j, 0]
                S = S + X[:, j, 1:]
                sq = sq + X[:, j, 1:] * X[:, j, 1:]
            inter = S * S - (T(0) if mut == "no_self_term" else sq)
            z = zw + T(0.5) * inter.sum(1)
        yy = y.astype(T)
        g = T(1) / (T(1) + np.exp(-z)) - yy
        loss = np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z))) - yy * z
        self.losses.append(loss.astype(np.float64))
        self.zmax = max(self.zmax, float(np.abs(z).max()))
        # per-key gradient
        go, vo = g[s], R[inv][:, 1:]
        keep = np.ones(len(s), bool)
        if mut == "wave_tail":  # lists longer than kFmLong lose their last count mod 64
            c = cnt[inv]
            keep = ~((c > KFM_LONG) & (_occ_rank(inv) >= c - c % 64))
        G = np.empty((nu, D), T)
        G[:, 0] = self._sum(inv[keep], go[keep], nu)
        gss = g[:, None] * S                       # [nb, K]
        if mut == "gss_stride":  # the sample's gss row read at stride DIM
            flat = gss.reshape(-1)
            gss_o = flat[(s[:, None] * D + np.arange(K)[None, :]) % len(flat)]
        else:
            gss_o = gss[s]
        factored = self.form == "factored" or mut in ("v_not_subtracted", "v_once_per_key",
                                                      "gss_stride")
        for f in range(K):
            if factored:
                Gs = self._sum(inv[keep], gss_o[keep, f], nu)
                sub = (T(0) if mut == "v_not_subtracted" else
                       R[:, 1 + f] if mut == "v_once_per_key" else R[:, 1 + f] * G[:, 0])
                G[:, 1 + f] = Gs - sub
            else:
                G[:, 1 + f] = self._sum(inv[keep], (go * (S[s, f] - vo[:, f]))[keep], nu)
        # the bound, from the reference's own quantities
        eG = grad_bound(X, s, inv, R, g, nu)
        # the update, once per key
        lr, x, h = T(self.lr), self.x[pos], self.h[pos]
        if mut == "per_occurrence":
            terms = np.concatenate([go[:, None], go[:, None] * (S[s] - vo)], axis=1)
            x, h = self._per_occurrence(x, h, inv, terms)
        else:
            x, h = update(self.opt, self.lr, x, h, G, T)
        hs = np.roll(h, 1, axis=1) if mut == "h_shifted" else h  # h block one column off
        self.x[pos], self.h[pos] = x, hs
        dx, dh, ill = update_bound(self.opt, self.lr, h, G, eG)
        self.ill += int(ill.any(1).sum())
        self.dx[pos] += dx
        self.dh[pos] += dh
        return loss

    def _per_occurrence(self, x, h, inv, terms):
        """The mutant update: once per occurrence, in occurrence order."""
        rank = _occ_rank(inv)
        by = np.argsort(rank, kind="stable")
        ends = np.searchsorted(rank[by], np.arange(rank.max() + 2))
        x, h, lr = x.copy(), h.copy(), self.T(self.lr)
        for r in range(len(ends) - 1):
            sel = by[ends[r]:ends[r + 1]]
            kk, t = inv[sel], terms[sel]
            if self.opt == "adagrad":
                h[kk] += t * t
                x[kk] -= lr * t / np.sqrt(h[kk] + self.T(EPS))
            else:
                x[kk] -= lr * t
        return x, h

    def result(self) -> Result:
        x, h = self.x.astype(np.float64), self.h.astype(np.float64)
        return Result(self.keys.copy(), x, h, 1e-6 + 1e-4 * np.abs(x) + self.dx,
                      1e-7 + 1e-4 * h + self.dh, self.losses, self.ill, self.zmax)


def batches(name: str, world: int = 1, steps: int = STEPS):
    """Per step the union batch (keys, y) of ``world`` ranks (B / world rows
    each, concatenated in rank order): a synchronous round's batch."""
    ds = dataset(name)
    out = []
    for t in range(steps):
        parts = [ds.batch(t, B // world, r, world) for r in range(world)]
        out.append(tuple(np.concatenate([p[i] for p in parts]) for i in (0, 2)))
    return out


def default_lr(name: str, optimizer: str) -> float:
    return HOT_SGD_LR if (name == "fm_hot" and optimizer == "sgd") else LR[optimizer]


def run(name: str, optimizer: str, K: int, world: int = 1, **kw) -> Result:
    kw.setdefault("lr", default_lr(name, optimizer))
    orc = FMOracle(K, optimizer, **kw)
    for k, y in batches(name, world):
        orc.step(k, y)
    return orc.result()


@functools.lru_cache(maxsize=None)
def reference(name: str, optimizer: str, K: int, world: int = 1) -> Result:
    """The fp64 reference of a data set, optimizer and K, computed once and
    shared (read-only) by every test that needs it."""
    r = run(name, optimizer, K, world)
    for a in (r.keys, r.x, r.h, r.tol_x, r.tol_h):
        a.setflags(write=False)
    return r


def ratios(res: Result, keys: np.ndarray, x: np.ndarray, h: np.ndarray | None = None):
    """(max |x - ref| / tol_x, max |h - ref| / tol_h, share of keys with any
    coordinate outside) of a model over exactly ``res.keys`` (any order, each
    once)."""
    order = np.argsort(keys)
    keys = keys[order]
    assert len(keys) == len(res.keys) and np.array_equal(keys, res.keys), (len(keys), len(res.keys))
    rx = np.abs(x[order].astype(np.float64) - res.x) / res.tol_x
    rh = (np.abs(h[order].astype(np.float64) - res.h) / res.tol_h if h is not None
          else np.zeros_like(rx))
    return float(rx.max()), float(rh.max()), float(((rx > 1) | (rh > 1)).any(1).mean())


class Stepwise:
    """Holds a model under test to the oracle one step at a time.

    Before each step the oracle takes the model's own state (``rebase``),
    computes the step in fp64 with this step's bound, and the model's state
    after the step must sit within ``1e-6 + 1e-4 |x| + dx_t`` (``tol_h``
    alike) for every key the batch touched, and be bit-identical for every
    other key.  The model's state then becomes the next step's start, so no
    error is carried and nothing can hide behind a carried bound.  ``last`` is
    the oracle's ``Result`` of the latest step, ``keys`` / ``x`` / ``h`` the
    model's state after it in the same (sorted) order."""

    def __init__(self, K: int, optimizer: str, lr: float | None = None, init_rows=None):
        self.orc = FMOracle(K, optimizer, lr=lr, init_rows=init_rows)
        self.keys = np.empty(0, np.uint64)
        self.x = self.h = np.empty((0, 1 + K))
        self.rx = self.rh = self.out = 0.0

    @property
    def ill(self) -> int:
        return self.orc.ill

    @property
    def losses(self) -> list:
        return self.orc.losses

    def step(self, bkeys, y, keys, x, h=None, pulled=None):
        """One step on the batch (``bkeys``, ``y``); (``keys``, ``x``, ``h``):
        the model's state after it (any order, each key once)."""
        o = self.orc
        o.rebase(self.keys, self.x, self.h)
        o.step(bkeys, y, pulled=pulled)
        r = o.result()
        order = np.argsort(keys)
        keys, x = keys[order], x[order].astype(np.float64)
        h = h[order].astype(np.float64) if h is not None else np.zeros_like(x)
        assert len(keys) == len(r.keys) and np.array_equal(keys, r.keys), (len(keys), len(r.keys))
        same = ~o.dx.any(1)  # keys the batch did not touch
        assert np.array_equal(x[same], r.x[same]) and np.array_equal(h[same], r.h[same])
        rx, rh = np.abs(x - r.x) / r.tol_x, np.abs(h - r.h) / r.tol_h
        self.rx, self.rh = max(self.rx, float(rx.max())), max(self.rh, float(rh.max()))
        self.out = max(self.out, float(((rx > 1) | (rh > 1)).any(1).mean()))
        self.keys, self.x, self.h, self.last = keys, x, h, r
        return float(rx.max()), float(rh.max())


def stepwise(name: str, optimizer: str, K: int, world: int = 1, **kw) -> Stepwise:
    """A free-running model (an ``FMOracle`` in fp32, or with a mutant) held
    to the oracle step by step."""
    lr = default_lr(name, optimizer)
    model = FMOracle(K, optimizer, lr=lr, **kw)
    sw = Stepwise(K, optimizer, lr)
    for k, y in batches(name, world):
        model.step(k, y)
        sw.step(k, y, model.keys, model.x, model.h)
    sw.model = model
    return sw


def key_gradient(uid: np.ndarray, rows: np.ndarray, y: np.ndarray):
    """The fp64 gradient rows of one batch and their bound, for the
    kernel-level tests: ``uid`` [B, F] is each occurrence's unique row (-1:
    none), ``rows`` [n, 1 + K] the unique rows, ``y`` [B] the labels.  Returns
    (G, eG, cnt): per unique row the gradient ``[G_w | G_f]``, the bound
    ``[eG_w | eG_f]`` of the module docstring, and the occurrence count (rows
    with none have G = eG = 0)."""
    nb, nf = uid.shape
    n, D = rows.shape
    K = D - 1
    mask = uid >= 0
    s, inv = np.nonzero(mask)[0], uid[mask]
    R = rows.astype(np.float64)
    X = np.zeros((nb, nf, D))
    X[mask] = R[inv]
    S = X[..., 1:].sum(1)
    z = X[..., 0].sum(1) + 0.5 * ((S * S).sum(1) - (X[..., 1:] ** 2).sum((1, 2)))
    g = 1.0 / (1.0 + np.exp(-z)) - y.astype(np.float64)
    go, vo = g[s], R[inv][:, 1:]
    cnt = np.bincount(inv, minlength=n)
    G = np.empty((n, D))
    G[:, 0] = np.bincount(inv, go, minlength=n)
    for f in range(K):
        G[:, 1 + f] = np.bincount(inv, go * (S[s, f] - vo[:, f]), minlength=n)
    eG = grad_bound(X, s, inv, R, g, n)
    return G, eG, cnt
