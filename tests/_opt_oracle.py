"""The update-rule menu (SGD, AdaGrad, FTRL-Proximal, lazy Adam, with L1/L2,
a gradient scale and a clip) in fp64, with an error bound, planted inputs and
planted mutants.

Nothing here comes from ``ss/optim.h`` or ``ops/optim.py``: the rules are the
published per-coordinate definitions, written once over a small number type
(``N``) that carries a running error bound beside each value.

Definitions (one coordinate; ``g`` the merged gradient of the push)
------------------------------------------------------------------
Preamble, every rule:   g <- g * grad_scale ;  g <- clip(g, -clip, +clip)
(clip = 0: off); SGD, AdaGrad and Adam then take L2 into the gradient,
``g <- g + l2 * w``; FTRL takes it in its denominator instead.

    SGD        w <- w - lr g
    AdaGrad    n <- n + g^2 ;  w <- w - lr g / sqrt(n + eps)
    FTRL-Proximal (McMahan et al. 2013, per coordinate, w materialised)
               n' = n + g^2 ;  sigma = (sqrt(n') - sqrt(n)) / alpha
               z <- z + g - sigma w
               w <- 0                                   if |z| <= l1
                    -(z - sign(z) l1) / ((beta + sqrt(n')) / alpha + l2)  else
               n <- n'
    Adam (Kingma & Ba 2015), lazy
               m <- b1 m + (1 - b1) g ;  v <- b2 v + (1 - b2) g^2
               w <- w - lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)

*Lazy* Adam, the project's definition: a key's (m, v) move only in a round
that pushes the key, and ``t`` is the 1-based index of the round the table is
applying — the global count of rounds, the same for every key of the push,
not a per-key count of updates.  The first round a table ever applies has
t = 1, whatever keys it touches.

The hyperparameters are fp32 numbers (the device holds them so): ``Hyper.f32()``
rounds a configuration once, and the oracle computes in fp64 from those
values — ``1 - b1^t`` from the fp32 ``b1``, not from the decimal it was typed as.

The bound
---------
``N`` evaluates a formula in dtype T and, beside every value, an absolute
error bound e in fp64.  Inputs read from fp32 rows and fp32 gradients are
exact (e = 0).  With u = 2^-24 (fp32 unit round-off) and a floor
tiny = 2^-126 (a flushed or denormal result), every operation adds one
rounding of its result to the first-order propagation of its operands':

    x + y, x - y   e = ex + ey                       + u |r| + tiny
    x * y          e = |x| ey + |y| ex + ex ey       + u |r| + tiny
    x / y          e = (ex + |r| ey) / (|y| - ey)    + u |r| + tiny
    sqrt(x)        e = sqrt(x) - sqrt(max(x - ex, 0)) + u |r| + tiny
                       (= ex / (2 sqrt x) to first order, finite at x = 0)
    clip, the L1 shrink z -> z - sign(z) l1 (0 inside), negation:
                   1-Lipschitz selections, e = ex (the shrink's subtraction
                   rounds once; a value clipped with its whole interval
                   beyond the clip is +-clip exactly, e = 0)

What is and is not correctly rounded on the device was read, not assumed:
the HIP extension is built with ``-O3`` and no fast-math flag
(``_build.py``); hipcc's defaults for HIP keep ``/`` and ``sqrtf`` correctly
rounded (``-fhip-fp32-correctly-rounded-divide-sqrt`` is on unless switched
off; the gfx950 assembly of ``opt_update`` shows the ``v_div_scale`` /
``v_div_fmas`` / ``v_div_fixup`` sequence and the scaled ``v_sqrt`` with its
correction steps) and allow contraction into FMAs, which only removes
roundings.  The one exception is AdaGrad's ``__frsqrt_rn``: correctly rounded
by name only — the compiler's HIP math header defines it as
``__builtin_amdgcn_rsqf``, the hardware ``V_RSQ_F32``, documented at 1 ulp =
2^-23 relative.  AdaGrad's square root is therefore charged ``RSQ = 2 u``
and the division that follows one more u for the product with the reciprocal
(the host's ``1.0f / sqrt`` then a product is three roundings: the same
charge).  ``1 - b`` is one rounding; the bias corrections are
computed on the host in fp64 and rounded once to fp32 (u each).

Per rule this gives, to first order (c = the clipped, scaled gradient, u
factors of the final w only):
    SGD      dw = u (|c| [scale] + |l2 w| + 2 |g| [the L2 product and sum]) lr
                  + u |lr g| + u |w'|
    AdaGrad  dn = 2 |g| dg + u (g^2 + n') ;  dw as SGD with the step
             multiplied by 1/sqrt(n' + eps) and charged dn / (2 (n' + eps))
             + 3 u relative besides
    FTRL     dsigma = (u (2 sqrt n' + sqrt n) + dn' / (2 sqrt n')) / alpha
             + 2 u |sigma|: the cancellation in sqrt(n') - sqrt(n) makes it
             about u sqrt(n) / alpha absolute, however small sigma
             ~ g^2 / (2 alpha sqrt n) is when g^2 << n.  dz = dg + |w| dsigma
             + u (|sigma w| + |g - sigma w| + |z'|);  dw = dz / D + |w'| dD / D
             + 3 u |w'| with D the denominator.
    Adam     dm = b1-product, (1 - b1) and the sum: about 4 u |m'| + (1 - b1) dg;
             dv likewise with 2 |g| dg;  dw = lr (dmhat / den + |mhat| dden /
             den^2) + 3 u |step| + u |w'|, den = sqrt(vhat) + eps.
The code does not use these closed forms: it runs the table above through
the formula, so no constant is chosen by hand.

A correctly rounded fp32 evaluation attains a first-order worst case, so a
check at exactly that sum would leave a correct kernel no headroom (a single
rounding already reaches u |r| when r sits just above a power of two).  The
bound is ``SAFETY = 2`` times the running sum: a correct fp32 evaluation in
any operation order stays within *half* the bound, and that is what
``test_opt_oracle_cpu.py`` checks of this module's own fp32 evaluation.  The
factor comes from that reasoning and the CPU calibration, not from a kernel.
Measured there (largest |fp32 - fp64| / bound over every planted and
Gaussian coordinate, six steps, plain and regularised settings):

    plain        sgd 0.468   adagrad 0.485   ftrl 0.494   adam 0.487
    regularised  sgd 0.455   adagrad 0.489   ftrl 0.497   adam 0.489

(parameters and states together; each test prints its own as ``CALIBRATION
...``).  They sit just under 0.5 because a single rounding of a result just
above a power of two is worth half the bound by itself; the MI355X's figures
(``test_gpu_opt_oracle.py``, ``docs/TESTING.md``) are the same 0.40-0.50.

Free-running trajectories (SGD, Adam) carry e from step to step through the
same propagation, so their bound grows with the steps taken.

bf16 rows: the math is fp32 on values that are exactly representable, and the
store rounds stochastically, so a stored word is one of the two bf16
neighbours of the fp32 result: ``bf16_interval`` gives the bf16 numbers
bracketing [oracle - bound, oracle + bound].  Where the bound is 0 and the
oracle is representable the two coincide: the value must come back exactly.

Mutants (``MUTANTS``): one-line wrong variants of the rules.  Each must
leave the bound on at least one planted coordinate.  ``ftrl_lt`` (``|z| <
l1``) has the same *value* everywhere, w being continuous at the threshold:
it differs in yielding -0.0 where the rule says 0 for z = +l1 exactly, and
``ratio`` counts a zero of the wrong sign in FTRL's w as outside the bound.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

U = 2.0 ** -24      # fp32 unit round-off
RSQ = 2.0           # roundings charged to 1/sqrt (V_RSQ_F32: 1 ulp = 2 u)
TINY = 2.0 ** -126  # smallest normal fp32: a flushed or denormal result
SAFETY = 2.0
KINDS = ("sgd", "adagrad", "ftrl", "adam")
NSTATE = {"sgd": 0, "adagrad": 1, "ftrl": 2, "adam": 2}
MUTANTS = {
    "clip_before_scale": KINDS, "l2_before_clip": ("sgd", "adagrad", "adam"),
    "t_lag": ("adam",), "no_bias_correction": ("adam",),
    "ftrl_lt": ("ftrl",), "ftrl_no_sign": ("ftrl",), "ftrl_no_l2": ("ftrl",),
    "ftrl_sigma_n2": ("ftrl",), "adam_eps_inside": ("adam",), "adagrad_eps_outside": ("adagrad",),
}


@dataclass(frozen=True)
class Hyper:
    kind: str = "sgd"
    lr: float = 0.1
    l1: float = 0.0
    l2: float = 0.0
    eps: float = 1e-8
    beta1: float = 0.9
    beta2: float = 0.999
    ftrl_alpha: float = 0.05
    ftrl_beta: float = 1.0
    grad_scale: float = 1.0
    clip: float = 0.0

    def f32(self) -> "Hyper":
        """The same configuration with every number rounded to fp32."""
        return replace(self, **{k: float(np.float32(v)) for k, v in self.__dict__.items()
                                if k != "kind"})

    def kwargs(self) -> dict:
        return dict(self.__dict__)


# --------------------------------------------------------- number with bound
class N:
    """A value (dtype T) with a running absolute error bound (fp64);
    ``e = None``: the value alone (no operand of the result carried one)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v)
        self.e = None if e is None else np.zeros(self.v.shape) + e

    @property
    def T(self):
        return self.v.dtype.type

    def _lift(self, o) -> "N":
        return o if isinstance(o, N) else N(self.T(o), None if self.e is None else 0.0)

    @staticmethod
    def _rnd(v, e, k=1.0) -> "N":
        if e is None:
            return N(v, None)
        return N(v, e + k * U * np.abs(v.astype(np.float64)) + TINY)

    def __add__(self, o):
        o = self._lift(o)
        return N._rnd(self.v + o.v, None if self.e is None else self.e + o.e)

    def __sub__(self, o):
        o = self._lift(o)
        return N._rnd(self.v - o.v, None if self.e is None else self.e + o.e)

    def __mul__(self, o):
        o = self._lift(o)
        if self.e is None:
            return N(self.v * o.v, None)
        a, b = np.abs(self.v.astype(np.float64)), np.abs(o.v.astype(np.float64))
        return N._rnd(self.v * o.v, a * o.e + b * self.e + self.e * o.e)

    __radd__, __rmul__ = __add__, __mul__

    def __rsub__(self, o):
        return self._lift(o) - self

    def __truediv__(self, o):
        o = self._lift(o)
        r = self.v / o.v
        if self.e is None:
            return N(r, None)
        den = np.abs(o.v.astype(np.float64)) - o.e
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(den > 0, (self.e + np.abs(r.astype(np.float64)) * o.e) / den, np.inf)
        return N._rnd(r, e)

    def __neg__(self):
        return N(-self.v, self.e)

    def sqrt(self, k=1.0):
        if self.e is None:
            return N(np.sqrt(self.v), None)
        x = self.v.astype(np.float64)
        return N._rnd(np.sqrt(self.v), np.sqrt(x) - np.sqrt(np.maximum(x - self.e, 0.0)), k)

    def clip(self, c):
        v = np.clip(self.v, -self.T(c), self.T(c))
        if self.e is None:
            return N(v, None)
        # a value whose whole interval lies beyond the clip is +-c exactly
        return N(v, np.where(np.abs(self.v.astype(np.float64)) - self.e >= float(self.T(c)),
                             0.0, self.e))

    def const(self, c, roundings=0.0):
        """A host-computed constant, rounded ``roundings`` times on its way
        to the device."""
        v = np.full(self.v.shape, self.T(c))
        return N(v, None if self.e is None else roundings * U * abs(float(c)))


def as_n(x, T=np.float64, track=True) -> N:
    if isinstance(x, N):
        return N(x.v.astype(T), x.e if track else None)
    return N(np.asarray(x).astype(T), 0.0 if track else None)


# ------------------------------------------------------------------- rules
def _gradient(h: Hyper, w: N, g: N, mutant, l2: bool) -> N:
    if mutant == "clip_before_scale":
        g = (g.clip(h.clip) if h.clip > 0 else g) * h.grad_scale
    elif mutant == "l2_before_clip" and l2:
        g = g * h.grad_scale + w * h.l2
        return g.clip(h.clip) if h.clip > 0 else g
    else:
        g = g * h.grad_scale
        if h.clip > 0:
            g = g.clip(h.clip)
    return g + w * h.l2 if l2 else g


def sgd(h: Hyper, w: N, g: N, mutant=None):
    g = _gradient(h, w, g, mutant, True)
    return w - g * h.lr, None, None


def adagrad(h: Hyper, w: N, n: N, g: N, mutant=None):
    g = _gradient(h, w, g, mutant, True)
    n = n + g * g
    if mutant == "adagrad_eps_outside":
        return w - g * h.lr / (n.sqrt() + h.eps), n, None
    # the device multiplies by a 1-ulp reciprocal square root: the square
    # root is charged RSQ roundings, the division stands for the product
    return w - g * h.lr / (n + h.eps).sqrt(RSQ), n, None


def ftrl(h: Hyper, w: N, z: N, n: N, g: N, mutant=None):
    g = _gradient(h, w, g, mutant, False)
    n2 = n + g * g
    r2 = n2.sqrt()
    sigma = (r2 if mutant == "ftrl_sigma_n2" else r2 - n.sqrt()) / h.ftrl_alpha
    z = z + (g - sigma * w)
    T, l1 = z.T, z.T(h.l1)
    inside = (np.abs(z.v) < l1) if mutant == "ftrl_lt" else (np.abs(z.v) <= l1)
    sgn = T(1) if mutant == "ftrl_no_sign" else np.sign(z.v)
    # the shrink: a 1-Lipschitz selection and one subtraction
    shr = N._rnd(np.where(inside, T(0), z.v - sgn * l1), z.e)
    den = (r2 + h.ftrl_beta) / h.ftrl_alpha
    if mutant != "ftrl_no_l2":
        den = den + h.l2
    q = -(shr / den)
    return N(np.where(inside, T(0), q.v), q.e), z, n2


def adam(h: Hyper, w: N, m: N, v: N, g: N, t: int, mutant=None):
    g = _gradient(h, w, g, mutant, True)
    one = g.const(1.0)
    m = m * h.beta1 + (one - h.beta1) * g
    v = v * h.beta2 + (one - h.beta2) * g * g
    if mutant == "t_lag":
        t = max(1, t - 1)
    bc1, bc2 = 1.0 / (1.0 - h.beta1 ** t), 1.0 / (1.0 - h.beta2 ** t)
    if mutant == "no_bias_correction":
        bc1 = bc2 = 1.0
    mh, vh = m * g.const(bc1, 1), v * g.const(bc2, 1)
    den = (vh + h.eps).sqrt() if mutant == "adam_eps_inside" else vh.sqrt() + h.eps
    return w - mh * h.lr / den, m, v


def step(h: Hyper, w, s1, s2, g, t: int = 1, T=np.float64, mutant=None, track=True):
    """One step of rule ``h.kind`` on every coordinate: ``(w, s1, s2)`` after
    it as ``N`` (states a rule does not have: ``None``).  ``t``: the 1-based
    round (Adam).  Inputs: arrays (exact) or ``N`` (a trajectory's running
    bound goes on).  T = float32 evaluates the same formula with every
    operation rounded to fp32.  ``track=False``: the values alone."""
    assert mutant is None or h.kind in MUTANTS[mutant], (mutant, h.kind)
    w, g = as_n(w, T, track), as_n(g, T, track)
    if h.kind == "sgd":
        return sgd(h, w, g, mutant)
    if h.kind == "adagrad":
        return adagrad(h, w, as_n(s1, T, track), g, mutant)
    if h.kind == "ftrl":
        return ftrl(h, w, as_n(s1, T, track), as_n(s2, T, track), g, mutant)
    return adam(h, w, as_n(s1, T, track), as_n(s2, T, track), g, t, mutant)


def bound(x: N) -> np.ndarray:
    return SAFETY * x.e


def ratio(ref: N, got: np.ndarray, ftrl_w: bool = False) -> np.ndarray:
    """|got - ref| / bound per coordinate (0 where both the difference and
    the bound are 0; inf where only the bound is).  ``ftrl_w``: a zero of the
    wrong sign where the rule says ``w = 0`` is outside."""
    d = np.abs(np.asarray(got, np.float64) - ref.v.astype(np.float64))
    b = bound(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / b)
    r = np.where(np.isnan(np.asarray(got, np.float64)), np.inf, r)
    if ftrl_w:
        z = (ref.v == 0) & (np.asarray(got) == 0)
        r = np.where(z & (np.signbit(got) != np.signbit(ref.v)), np.inf, r)
    return r


# ----------------------------------------------------------- rows of a table
def split(kind: str, rows: np.ndarray, dim: int):
    """(w, s1, s2) views [n, dim] of full rows [n, width]."""
    ns = NSTATE[kind]
    return (rows[:, :dim], rows[:, dim:2 * dim] if ns > 0 else None,
            rows[:, 2 * dim:3 * dim] if ns > 1 else None)


def join(parts) -> np.ndarray:
    return np.concatenate([p for p in parts if p is not None], axis=1)


def step_rows(h: Hyper, rows, grads, dim: int, t: int = 1, T=np.float64, mutant=None):
    """``step`` on full rows: (values [n, width], bounds [n, width], N parts)."""
    w, s1, s2 = split(h.kind, rows, dim) if not isinstance(rows, tuple) else rows
    out = step(h, w, s1, s2, grads, t, T, mutant)
    return join([None if p is None else p.v for p in out]), \
        join([None if p is None else bound(p) for p in out]), out


def rows_ratio(h: Hyper, parts, got: np.ndarray, dim: int) -> np.ndarray:
    """``ratio`` of full rows ``got`` [n, width] against ``step``'s parts."""
    gw, g1, g2 = split(h.kind, got, dim)
    return join([ratio(parts[0], gw, ftrl_w=h.kind == "ftrl")] +
                [None if p is None else ratio(p, x) for p, x in ((parts[1], g1), (parts[2], g2))])


# ------------------------------------------------------------ bf16 neighbours
def bf16_floor(x: np.ndarray) -> np.ndarray:
    """Largest bf16 number <= x (x finite fp64), as fp32."""
    f = np.asarray(x, np.float64).astype(np.float32)
    f = np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f)
    b = f.astype(np.float32).view(np.uint32)
    trunc = (b & np.uint32(0xFFFF0000)).view(np.float32)   # toward zero
    down = ((b & np.uint32(0xFFFF0000)) + np.uint32(0x10000)).view(np.float32)  # away from zero
    exact = (b & np.uint32(0xFFFF)) == 0
    return np.where((f >= 0) | exact, trunc, down)


def bf16_interval(lo: np.ndarray, hi: np.ndarray):
    """The bf16 numbers bracketing [lo, hi]: (largest <= lo, smallest >= hi)."""
    return bf16_floor(lo), -bf16_floor(-np.asarray(hi, np.float64))


# ---------------------------------------------------------- planted inputs
def _f32(x):
    return np.asarray(x, np.float32)


def planted_grads(h: Hyper) -> np.ndarray:
    """fp32 gradients at the edges of the preamble: 0; g * grad_scale exactly
    at +-clip, one fp32 ulp inside, one outside, well outside; |g| of 1e-12
    and 1e4; a moderate pair.  Without a clip the same values around 1."""
    c = np.float32(h.clip if h.clip > 0 else 1.0)
    at = np.float32(c / np.float32(h.grad_scale))
    assert np.float64(at) * np.float64(np.float32(h.grad_scale)) == np.float64(c), \
        "planted clip edge: clip / grad_scale must be exact in fp32"
    pos = [at, np.nextafter(at, np.float32(0)), np.nextafter(at, np.float32(np.inf)),
           np.float32(37.5) * at, 1e4, 1e-12, 0.3, 0.0625]
    return _f32([0.0] + pos + [-x for x in pos])


def planted_states(h: Hyper):
    """fp32 row states (w, s1, s2) at the edges of rule ``h.kind``."""
    ws = [0.0, 0.25, -0.37, 0.0043]
    if h.kind == "sgd":
        return _f32(ws), None, None
    if h.kind == "adagrad":   # n: first touch, state_init, tiny, large, huge
        w, n = np.meshgrid(ws, [0.0, 0.05, 1e-10, 3.0, 1e6], indexing="ij")
        return _f32(w.ravel()), _f32(n.ravel()), None
    if h.kind == "adam":      # m = v = 0; ordinary; eps dominates sqrt(v); large
        mv = [(0.0, 0.0), (0.01, 1e-4), (1e-10, 1e-20), (-1e-9, 4e-18), (-0.3, 2.0)]
        w = np.repeat(ws, len(mv))
        m, v = np.tile([a for a, _ in mv], len(ws)), np.tile([b for _, b in mv], len(ws))
        return _f32(w), _f32(m), _f32(v)
    # ftrl: first touch (n = 0) from zero and uniform init; n >> g^2; ordinary
    # states, consistent (w materialised from (z, n)) and not
    rows = [(0.0, 0.0, 0.0), (0.0043, 0.0, 0.0), (-0.0021, 0.0, 0.0),
            (0.25, -6.0, 1e6), (-0.37, 9.0, 1e6), (0.0, 0.01, 1e6), (0.25, 1.0, 1e10),
            (0.25, -0.8, 0.5), (-0.37, 0.3, 2.0), (0.0, 0.02, 0.5)]
    l1 = np.float64(np.float32(h.l1))
    for zz, nn in ((-2.0, 0.7), (1.3, 4.0)):   # consistent rows
        r2 = np.sqrt(nn)
        ww = 0.0 if abs(zz) <= l1 else -(zz - np.sign(zz) * l1) / (
            (h.ftrl_beta + r2) / h.ftrl_alpha + h.l2)
        rows.append((ww, zz, nn))
    w, z, n = (np.array([r[i] for r in rows]) for i in range(3))
    return _f32(w), _f32(z), _f32(n)


def planted_threshold(h: Hyper):
    """FTRL coordinates (w, z, n, g) whose z' lands exactly on +-l1, one fp32
    ulp of z to either side (inside the bound), and far from it.  w = 0, so
    z' = z + g' exactly (g' the scaled gradient), checked here in fp64."""
    s, l1 = np.float32(h.grad_scale), np.float32(h.l1)
    g = np.float32(0.0625)
    ge = np.float64(g) * np.float64(s)
    assert h.clip == 0 or ge < h.clip
    z0 = np.float32(np.float64(l1) - ge)
    assert np.float64(z0) + ge == np.float64(l1), "planted threshold is not exact"
    out = []
    for sign in (1.0, -1.0):
        for z in (z0, np.nextafter(z0, np.float32(np.inf)), np.nextafter(z0, np.float32(-np.inf)),
                  np.float32(z0 + 1), np.float32(z0 - 1)):
            for n in (0.0, 0.5):
                out.append((0.0, sign * z, n, sign * g))
    a = _f32(out)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]


def planted(h: Hyper):
    """Every planted state crossed with every planted gradient (and FTRL's
    threshold coordinates): flat fp32 arrays (w, s1, s2, g)."""
    g = planted_grads(h)
    w, s1, s2 = planted_states(h)
    k, n = len(g), len(w)
    rep = lambda a: None if a is None else np.repeat(a, k)  # noqa: E731
    W, S1, S2, G = rep(w), rep(s1), rep(s2), np.tile(g, n)
    if h.kind == "ftrl":
        tw, tz, tn, tg = planted_threshold(h)
        W, S1, S2, G = (np.concatenate(p) for p in ((W, tw), (S1, tz), (S2, tn), (G, tg)))
    return W, S1, S2, G


def gaussian(h: Hyper, n: int, seed: int = 0):
    """Seeded ordinary coordinates: (w, s1, s2, g) fp32."""
    rng = np.random.default_rng(seed)
    w = _f32(rng.uniform(-0.25, 0.25, n))
    g = _f32(rng.standard_normal(n))
    pos = lambda: _f32(rng.uniform(0.0, 2.0, n) ** 2)  # noqa: E731
    if h.kind == "sgd":
        return w, None, None, g
    if h.kind == "adagrad":
        return w, pos(), None, g
    if h.kind == "ftrl":
        return w, _f32(rng.standard_normal(n)), pos(), g
    return w, _f32(0.1 * rng.standard_normal(n)), _f32(0.01 * pos()), g


def fill(a, shape, roll: int = 0) -> np.ndarray:
    """``a`` tiled (and rolled) over an fp32 array of ``shape``."""
    if a is None:
        return None
    n = int(np.prod(shape))
    return np.resize(np.roll(a, roll), n).reshape(shape).astype(np.float32)


def table_rows(h: Hyper, nkeys: int, dim: int, seed: int = 0) -> np.ndarray:
    """Initial full rows [nkeys, width]: the planted states crossed with the
    planted gradients of ``table_grads(step 0)`` on the first coordinates,
    seeded ordinary states on the rest."""
    pw, p1, p2, _ = planted(h)
    gw, g1, g2, _ = gaussian(h, nkeys * dim, seed)
    k = min(len(pw), nkeys * dim)
    out = []
    for p, g in ((pw, gw), (p1, g1), (p2, g2)):
        if p is not None:
            g = g.copy()
            g[:k] = p[:k]
            out.append(g.reshape(nkeys, dim))
    return np.concatenate(out, axis=1)


def table_grads(h: Hyper, nkeys: int, dim: int, step_no: int, seed: int = 0) -> np.ndarray:
    """Gradients [nkeys, dim] of step ``step_no``: even steps the planted
    gradients (aligned with ``table_rows``' planted states at step 0, rolled
    by the step after), odd steps seeded Gaussian."""
    if step_no % 2:
        return _f32(np.random.default_rng(1000 + 17 * seed + step_no).standard_normal((nkeys, dim)))
    g = planted(h)[3]
    return fill(g, (nkeys, dim), roll=0 if step_no == 0 else 7 * step_no + 1)


SETTINGS = {
    # plain: no regularisation, scale 1;  reg: what the rule has of L1/L2, a
    # scale of 1/2 and a clip (clip / scale exact in fp32)
    ("sgd", "plain"): Hyper("sgd", lr=0.1),
    ("sgd", "reg"): Hyper("sgd", lr=0.1, l2=0.01, grad_scale=0.5, clip=1.0),
    ("adagrad", "plain"): Hyper("adagrad", lr=0.1),
    ("adagrad", "reg"): Hyper("adagrad", lr=0.1, l2=0.01, grad_scale=0.5, clip=1.0),
    ("ftrl", "plain"): Hyper("ftrl"),
    ("ftrl", "reg"): Hyper("ftrl", l1=0.0625, l2=0.01, grad_scale=0.5, clip=1.0),
    ("adam", "plain"): Hyper("adam", lr=0.01),
    ("adam", "reg"): Hyper("adam", lr=0.01, l2=0.01, grad_scale=0.5, clip=1.0),
}


def setting(kind: str, which: str) -> Hyper:
    return SETTINGS[(kind, which)].f32()
