"""A high-precision sparse-LR reference with an error bound, and its data.

Nothing here comes from the engine: the data sets are drawn from a seeded
NumPy generator and written as libsvm text, so the loaders and this module
see byte-identical input; the model is a dozen lines of NumPy in fp64; the
only project code used is ``init_reference``, the host mirror of the
key-seeded initialiser (as ``test_gpu_oracle.py`` does).

Data sets (``dataset(name)``; B = 4096, F = 13, 8 steps = 32768 rows)
---------------------------------------------------------------------
* ``binary32``: ``label idx idx ...``; every key below 2^32 (the route moves
  8-byte records).
* ``valued64``: ``label idx:val ...`` with ``val = +-U(0.25, 2)`` rounded to
  the four decimals the text prints; a quarter of the distinct indices carry
  bits at or above 2^32 (12-byte records).

Rows hold 3..F entries, a few rows none; short rows are padded with the EMPTY
key (value 0).  Indices are ``zipf(1.3) * 7919 % 2_000_003 + 1``: a hot head
(the hottest key has thousands of occurrences per batch, several in one
row), duplicates and ~20k distinct keys, most of them singletons.  Labels are
Bernoulli draws of a planted model.

The model (``LROracle``), per step over the batch's non-EMPTY entries
--------------------------------------------------------------------
    z_s = sum_j w[k_sj] * x_sj
    g_s = sigmoid(z_s) - y_s
    loss_s = max(z_s, 0) + log1p(exp(-|z_s|)) - y_s * z_s
    G_k = sum over the occurrences (s, j) of k of g_s * x_sj
    adagrad:  h_k += G_k^2 ;  w_k -= lr * G_k / sqrt(h_k + eps)
    sgd:      w_k -= lr * G_k
once per key and step; a key seen for the first time starts from
``init_reference`` (uniform, scale 0.01; h = 0).
FTRL-Proximal, lazy Adam and the regularised settings (L1 / L2, clip, scale)
step by ``_opt_oracle.step`` instead, on fp32 hyperparameters, the gradient
entering it known to eG and the bound it carries taking the place of the
dw / dh sums below (``OPT_SETTINGS``; ``test_gpu_opt_oracle.py``).

The error bound carried beside the state
----------------------------------------
For key k at step t with occurrences O and A = sum_O |g_s x_sj|:

    eG   = u_g * A + 2^-24 * |O| + |O| * 2^-24 * A
    adagrad:  dw_t = lr * eG / sqrt(h_after + eps),  dh_t = 2 |G| eG + eG^2
    sgd:      dw_t = lr * eG
    tol_w = 1e-6 + 1e-4 |w| + sum_t dw_t
    tol_h = 1e-7 + 1e-4  h  + sum_t dh_t

2^-24 is the fp32 unit round-off: ``|O| 2^-24 A`` bounds any fp32 summation
order of |O| terms, ``2^-24 |O|`` the absolute error of each term (p = 1 /
(1 + e^-z) is rounded to fp32 before ``p - y``, half an ulp of a number below
1, times |x| <= 2; the fp32 sum z adds a like amount).  ``u_g`` is the
relative accuracy of one gradient term:

    u_g = 2^-21.

Where it comes from: the kernels compute p with ``__expf``.  Neither the HIP
headers nor the documents shipped with ROCm state its error; the compiler's
HIP math header (``__clang_hip_math.h``) defines it as
``__builtin_amdgcn_exp2f(0x1.715476p+0f * x)``: the hardware exp2
(``V_EXP_F32``; taken as 1 ulp = 2^-23 relative, the figure AMD's public ISA
documents give for it — the headers give none) of a product whose two
roundings (the constant, the multiply) move exp2's argument by up to
|x| log2(e) 2^-23, i.e. e^-z by a further |z| 2^-23 relative.  Through
g = sigmoid(z) - y a relative error r of e^-z moves g by p (1 - p) r:
    hardware exp2 ulp, the division and the addition:  <= 2 * 2^-23 |g|
    the argument's roundings:  (|z| p (1 - p)) 2^-23 <= 0.23 * 2^-23 for
    every z — an absolute amount, inside the 2^-24 per occurrence above.
So 2^-21 = 4 * 2^-23 holds the relative part with a factor 2 to spare for
any z (the oracle records the largest |z| it met, ``zmax``: 2.1 with
AdaGrad, 25 with SGD on binary32, whose hot key oscillates).  ``__logf``
(``__builtin_logf``) enters the loss only.

No key is excused: a key-step is *ill-conditioned* when ``eG > 0.1 *
sqrt(h_after + eps)`` (AdaGrad; the gradient's uncertainty reaches a tenth of
the denominator, so the first-order bound no longer describes the step).  The
data sets have none (``Result.ill == 0``, asserted from the oracle alone
before anything is compared with it); a seed that produced one would be
changed, not the rule.  SGD has no denominator and no such key-steps.

Measured (``test_lr_oracle_cpu.py``): the same model evaluated in fp32 with
the occurrence order permuted, three permutations, max |fp32 - fp64| / tol:

    binary32  adagrad  w 0.039  h 0.166      sgd  w 0.046
    valued64  adagrad  w 0.016  h 0.051      sgd  w 0.015

(NumPy's ``exp``), median tol_w 6.1e-6 at median |w| 5.0e-2 with AdaGrad,
1.3e-6 at 2.5e-3 with SGD; 0 ill-conditioned key-steps.  On the MI355X the
largest |engine - oracle| / tol over every path of
``test_gpu_lr_paths_oracle.py`` was 0.062 for w and 0.167 for h (that
module's docstring has them per path): the kernels' fast ``exp`` sits at the
fp32 noise floor, a sixth of the tolerance.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import _opt_oracle as _opt

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
B, F, STEPS = 4096, 13, 8
ROWS = B * STEPS
U32 = 2.0 ** -24   # fp32 unit round-off
U_G = 2.0 ** -21   # relative accuracy of one gradient term (module docstring)
LR = {"adagrad": 0.05, "sgd": 1e-3, "ftrl": 0.05, "adam": 0.01}   # (FTRL steps by ftrl_alpha)
INIT_SCALE, EPS = 0.01, 1e-8
SEEDS = {"binary32": 0, "valued64": 1}


# ------------------------------------------------------------------- data
@dataclass
class Dataset:
    name: str
    keys: np.ndarray    # [ROWS, F] uint64, EMPTY-padded
    x: np.ndarray       # [ROWS, F] float32, 0 at the padding
    y: np.ndarray       # [ROWS] float32
    lines: list = field(repr=False, default_factory=list)  # the libsvm text, one bytes per row

    @property
    def has_values(self) -> bool:
        return self.name == "valued64"

    def write(self, path) -> str:
        with open(path, "wb") as f:
            f.write(b"".join(self.lines))
        return str(path)

    def shard(self, rank: int = 0, world: int = 1) -> tuple[int, int]:
        """Rows [lo, hi) of rank's shard: the rank-th 1/world of the file's
        bytes, each cut moved forward to the next line start."""
        starts = np.concatenate([[0], np.cumsum([len(b) for b in self.lines])])
        size = int(starts[-1])
        cut = [int(np.searchsorted(starts, size * i // world)) for i in range(world)] + [ROWS]
        return cut[rank], cut[rank + 1]

    def batch(self, step: int, batch: int = B, rank: int = 0, world: int = 1):
        """(keys, x, y) of the shard's rows [step * batch, +batch), wrapping."""
        lo, hi = self.shard(rank, world)
        r = lo + (step * batch + np.arange(batch)) % (hi - lo)
        return self.keys[r], self.x[r], self.y[r]


@functools.lru_cache(maxsize=None)
def dataset(name: str) -> Dataset:
    rng = np.random.default_rng(SEEDS[name])
    valued = name == "valued64"
    n = rng.integers(3, F + 1, ROWS)
    n[rng.choice(ROWS, 7, replace=False)] = 0  # a few empty rows
    mask = np.arange(F)[None, :] < n[:, None]
    # zipf(1.3) * 7919 % 2_000_003 without overflowing int64
    idx = (rng.zipf(1.3, (ROWS, F)) % 2_000_003 * 7919 % 2_000_003 + 1).astype(np.uint64)
    if valued:  # a quarter of the indices above 2^32 (a function of the index)
        idx = np.where(idx % np.uint64(4) == 0, idx | ((idx % np.uint64(7) + np.uint64(1))
                                                       << np.uint64(32)), idx)
    keys = np.where(mask, idx, EMPTY)
    if valued:
        v = rng.uniform(0.25, 2.0, (ROWS, F)) * rng.choice([-1.0, 1.0], (ROWS, F))
        text = np.char.mod("%.4f", v)
        x = np.where(mask, text.astype(np.float64), 0.0).astype(np.float32)
    else:
        text = None
        x = mask.astype(np.float32)
    # labels from a planted model over the distinct keys
    u, inv = np.unique(keys, return_inverse=True)
    truth = rng.normal(0.0, 1.0, len(u))
    z = (truth[inv.reshape(ROWS, F)] * x).sum(1) - 0.5
    y = (rng.random(ROWS) < 1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    lines = []
    for r in range(ROWS):
        m = int(n[r])
        if valued:
            ent = [f"{int(k)}:{t}" for k, t in zip(keys[r, :m], text[r, :m])]
        else:
            ent = [str(int(k)) for k in keys[r, :m]]
        lines.append((" ".join([str(int(y[r]))] + ent) + "\n").encode())
    return Dataset(name, keys, x, y, lines)


# ----------------------------------------------------------------- update
def update(opt: str, lr, x, h, G, T=np.float64, h2=None, t: int = 1, **reg):
    """One optimizer step of every key, in ``T``: (x, h) after it — the one
    update of the LR, FM and word2vec oracles — by the rules of
    ``_opt_oracle.py``.  FTRL and Adam have a second state ``h2`` and return
    (x, h, h2); ``t`` is Adam's 1-based round; ``reg``: ``l1``, ``l2``,
    ``grad_scale``, ``clip`` and the rules' other hyperparameters."""
    hy = _opt.Hyper(opt, lr=lr, eps=EPS, **reg)
    w, s1, s2 = _opt.step(hy, x, h if opt != "sgd" else None, h2, G, t, T, track=False)
    if opt in ("sgd", "adagrad"):
        return w.v, (h if s1 is None else s1.v)
    return w.v, s1.v, s2.v


def update_bound(opt: str, lr, h_after, G, eG):
    """(dx, dh, ill) of one step (module docstring): what a gradient known to
    ``eG`` moves the parameters and the AdaGrad state by, and where the step
    is ill-conditioned."""
    if opt == "adagrad":
        den = np.sqrt(np.asarray(h_after, np.float64) + EPS)
        return (lr * eG / den, 2 * np.abs(np.asarray(G, np.float64)) * eG + eG * eG,
                eG > 0.1 * den)
    return lr * eG, np.zeros_like(eG), np.zeros(np.shape(eG), bool)


# ------------------------------------------------------------------ model
MUTANTS = ("x_one", "x_next", "drop_one", "dup_one", "per_occurrence")


@dataclass
class Result:
    keys: np.ndarray    # sorted, distinct
    w: np.ndarray
    h: np.ndarray       # zeros with sgd; FTRL's z, Adam's m
    tol_w: np.ndarray
    tol_h: np.ndarray
    losses: list        # per step: per-sample losses (fp64)
    ill: int            # ill-conditioned key-steps
    zmax: float
    h2: np.ndarray = None      # FTRL's n, Adam's v
    tol_h2: np.ndarray = None

    def mean_losses(self, world: int = 1) -> np.ndarray:
        """[steps, world]: each rank's mean loss (the batch is the ranks'
        batches concatenated)."""
        return np.array([l.reshape(world, -1).mean(1) for l in self.losses])


class LROracle:
    """Sparse LR over a sorted key set.  ``dtype`` float64 is the reference;
    float32 with ``perm`` (a seed) evaluates the same model in fp32 with the
    occurrence orders of both sums permuted (the noise floor).  ``mutant``
    plants one of ``MUTANTS``: each is a way a merge kernel can be subtly
    wrong."""

    def __init__(self, optimizer: str = "adagrad", lr: float | None = None, dtype=np.float64,
                 perm: int | None = None, mutant: str | None = None, **reg):
        from swiftsnails_amd.ops.optim import InitConfig

        assert optimizer in LR and mutant in (None,) + MUTANTS
        self.opt, self.lr = optimizer, LR[optimizer] if lr is None else lr
        # FTRL, Adam and the regularised settings (``reg``: l1, l2, clip,
        # grad_scale, ...) step by ``_opt_oracle.step`` on fp32 hyperparameters
        # and carry its running bound (the gradient enters it known to eG);
        # plain AdaGrad and SGD keep ``update`` / ``update_bound``
        self.general = optimizer in ("ftrl", "adam") or bool(reg)
        self.hy = _opt.Hyper(optimizer, lr=self.lr, eps=EPS, **reg).f32()
        self.t = 0
        self.h2, self.dh2 = np.empty(0, dtype), np.empty(0)
        self.T, self.mutant = dtype, mutant
        self.rng = np.random.default_rng(perm) if perm is not None else None
        self.init = InitConfig("uniform", INIT_SCALE)
        self.keys = np.empty(0, np.uint64)
        self.w, self.h = np.empty(0, dtype), np.empty(0, dtype)
        self.dw, self.dh = np.empty(0), np.empty(0)
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
            r = init_reference(self.init, new, 1, 2)
            keys = np.concatenate([self.keys, new])
            order = np.argsort(keys)
            z = np.zeros(len(new))
            self.keys = keys[order]
            self.w = np.concatenate([self.w, r[:, 0].astype(self.T)])[order]
            self.h = np.concatenate([self.h, r[:, 1].astype(self.T)])[order]
            self.dw = np.concatenate([self.dw, z])[order]
            self.dh = np.concatenate([self.dh, z])[order]
            self.h2 = np.concatenate([self.h2, z.astype(self.T)])[order]
            self.dh2 = np.concatenate([self.dh2, z])[order]
            pos = np.searchsorted(self.keys, u)
        return pos

    def step(self, keys: np.ndarray, x: np.ndarray, y: np.ndarray) -> np.ndarray:
        T, mut = self.T, self.mutant
        mask = keys != EMPTY
        s = np.nonzero(mask)[0]                    # sample of each occurrence
        u, first, inv = np.unique(keys[mask], return_index=True, return_inverse=True)
        pos = self._insert(u)
        xs = np.ones_like(x) if mut == "x_one" else x
        xo = xs[mask].astype(T)
        # forward: z over each row's entries (fp32: in a permuted field order)
        wf = np.zeros(keys.shape, T)
        wf[mask] = self.w[pos][inv]
        cols = self.rng.permutation(keys.shape[1]) if self.rng is not None else range(keys.shape[1])
        z = np.zeros(len(y), T)
        for j in cols:
            z = z + wf[:, j] * np.where(mask[:, j], xs[:, j], 0).astype(T)
        yy = y.astype(T)
        g = T(1) / (T(1) + np.exp(-z)) - yy
        loss = np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z))) - yy * z
        self.losses.append(loss.astype(np.float64))
        self.zmax = max(self.zmax, float(np.abs(z).max()))
        # per-key gradient
        if mut == "x_next":  # the merge reads the neighbouring occurrence's x
            xo = np.roll(xs.reshape(-1), -1).reshape(xs.shape)[mask].astype(T)
        term = g[s] * xo
        cnt = np.bincount(inv, minlength=len(u))
        if self.rng is not None:  # sequential fp32 sum in a permuted order
            order = self.rng.permutation(len(term))
            G = np.zeros(len(u), T)
            np.add.at(G, inv[order], term[order])
        else:
            G = np.bincount(inv, term, minlength=len(u)).astype(T)
        if mut in ("drop_one", "dup_one"):
            G = G + np.where(cnt > 1, term[first], 0) * (-1 if mut == "drop_one" else 1)
        A = np.bincount(inv, np.abs(term).astype(np.float64), minlength=len(u))
        eG = U_G * A + U32 * cnt + cnt * U32 * A
        # the update, once per key
        lr, w, h = T(self.lr), self.w[pos], self.h[pos]
        if self.general:
            return self._general_step(pos, G, eG, loss)
        if mut == "per_occurrence":
            w, h = self._per_occurrence(w, h, inv, term)
        else:
            w, h = update(self.opt, self.lr, w, h, G, T)
        self.w[pos], self.h[pos] = w, h
        dw, dh, ill = update_bound(self.opt, self.lr, h, G, eG)
        self.ill += int(ill.sum())
        self.dw[pos] += dw
        self.dh[pos] += dh
        return loss

    def _general_step(self, pos, G, eG, loss):
        """One round of ``_opt_oracle.step`` per key: the states go in with
        the bound they carry, the gradient with eG, and come out with both
        propagated (``dw`` / ``dh`` / ``dh2`` hold the running bound itself)."""
        ns = _opt.NSTATE[self.opt]
        self.t += 1
        w, s1, s2 = _opt.step(
            self.hy, _opt.N(self.w[pos], self.dw[pos]),
            _opt.N(self.h[pos], self.dh[pos]) if ns > 0 else None,
            _opt.N(self.h2[pos], self.dh2[pos]) if ns > 1 else None,
            _opt.N(G, eG), self.t, self.T)
        self.w[pos], self.dw[pos] = w.v, w.e
        if ns > 0:
            self.h[pos], self.dh[pos] = s1.v, s1.e
        if ns > 1:
            self.h2[pos], self.dh2[pos] = s2.v, s2.e
        self.ill += int((~np.isfinite(w.e)).sum())
        return loss

    def _per_occurrence(self, w, h, inv, term):
        """The mutant update: once per occurrence, in occurrence order."""
        order = np.argsort(inv, kind="stable")
        k = inv[order]
        rank = np.arange(len(k)) - np.searchsorted(k, k)   # occurrence number within its key
        by = np.argsort(rank, kind="stable")
        ends = np.searchsorted(rank[by], np.arange(rank.max() + 2))
        w, h, lr = w.copy(), h.copy(), self.T(self.lr)
        for r in range(len(ends) - 1):
            sel = order[by[ends[r]:ends[r + 1]]]
            kk, t = inv[sel], term[sel]
            if self.opt == "adagrad":
                h[kk] += t * t
                w[kk] -= lr * t / np.sqrt(h[kk] + self.T(EPS))
            else:
                w[kk] -= lr * t
        return w, h

    def result(self) -> Result:
        w, h = self.w.astype(np.float64), self.h.astype(np.float64)
        if self.general:
            h2, S = self.h2.astype(np.float64), _opt.SAFETY
            return Result(self.keys.copy(), w, h, 1e-6 + 1e-4 * np.abs(w) + S * self.dw,
                          1e-7 + 1e-4 * np.abs(h) + S * self.dh, self.losses, self.ill, self.zmax,
                          h2, 1e-7 + 1e-4 * np.abs(h2) + S * self.dh2)
        return Result(self.keys.copy(), w, h, 1e-6 + 1e-4 * np.abs(w) + self.dw,
                      1e-7 + 1e-4 * h + self.dh, self.losses, self.ill, self.zmax)


def batches(name: str, world: int = 1, steps: int = STEPS):
    """Per step the union batch of ``world`` ranks (B / world rows each,
    concatenated in rank order): a synchronous round's batch."""
    ds = dataset(name)
    out = []
    for t in range(steps):
        parts = [ds.batch(t, B // world, r, world) for r in range(world)]
        out.append(tuple(np.concatenate([p[i] for p in parts]) for i in range(3)))
    return out


def run(name: str, optimizer: str, world: int = 1, steps: int = STEPS, **kw) -> Result:
    orc = LROracle(optimizer, **kw)
    for k, x, y in batches(name, world, steps):
        orc.step(k, x, y)
    return orc.result()


@functools.lru_cache(maxsize=None)
def reference(name: str, optimizer: str, world: int = 1, steps: int = STEPS,
              reg: tuple = ()) -> Result:
    """The fp64 reference of a data set and optimizer (``reg``: the
    regularisation as sorted (name, value) pairs), computed once and shared
    (read-only) by every test that needs it."""
    r = run(name, optimizer, world, steps, **dict(reg))
    for a in (r.keys, r.w, r.h, r.tol_w, r.tol_h, r.h2, r.tol_h2):
        if a is not None:
            a.setflags(write=False)
    return r


# The rule settings the engine is held to (test_gpu_opt_oracle.py): rule and
# regularisation as ``reference``'s ``reg``; 4 steps each.
OPT_STEPS = 4
OPT_SETTINGS = {
    "ftrl_l1": ("ftrl", (("l1", 0.3),)),
    "adam": ("adam", ()),
    "adagrad_l2_clip": ("adagrad", (("clip", 1.0), ("l2", 0.01))),
    "sgd_l2": ("sgd", (("l2", 0.01),)),
}


def opt_reference(tag: str, name: str, world: int = 1) -> Result:
    opt, reg = OPT_SETTINGS[tag]
    return reference(name, opt, world, OPT_STEPS, reg)


def ftrl_near_threshold(res: Result, l1: float) -> np.ndarray:
    """Keys whose ``|z| - l1`` lies inside z's tolerance: the only keys whose
    ``w == 0`` may differ from the oracle's."""
    return np.abs(np.abs(res.h) - np.float64(np.float32(l1))) <= res.tol_h


def ratios(res: Result, keys: np.ndarray, w: np.ndarray, h: np.ndarray | None = None,
           h2: np.ndarray | None = None):
    """(max |w - ref| / tol_w, max |h - ref| / tol_h, share of keys outside
    either) of a model over exactly ``res.keys`` (any order, each once);
    ``h2``: the second state is held to ``tol_h2`` too, its ratio folded into
    the second figure."""
    order = np.argsort(keys)
    keys = keys[order]
    assert len(keys) == len(res.keys) and np.array_equal(keys, res.keys), (len(keys), len(res.keys))
    rw = np.abs(w[order].astype(np.float64) - res.w) / res.tol_w
    rh = (np.abs(h[order].astype(np.float64) - res.h) / res.tol_h if h is not None
          else np.zeros_like(rw))
    if h2 is not None:
        rh = np.maximum(rh, np.abs(h2[order].astype(np.float64) - res.h2) / res.tol_h2)
    return float(rw.max()), float(rh.max()), float(((rw > 1) | (rh > 1)).mean())
