"""``ftrl_zn`` (FTRL-Proximal in compact ``[z | n]`` rows) on the CPU: the
oracle helper held to itself, the host references held to it, and the public
surface that needs no GPU.

* ``_ftrl_zn_oracle``'s own fp32 evaluation of the pulled weight and of the
  step stays within half its bound on every planted and Gaussian coordinate,
  three rule settings, six steps taken one at a time from the fp32 rows (the
  criterion and ``SAFETY`` of ``test_opt_oracle_cpu.py``, nothing tuned);
* every planted mutant leaves the bound on a planted coordinate;
* ``apply_reference`` / ``pull_reference`` stay within the bound;
* ``ftrl_zn`` and ``ftrl`` (w materialised) from zero rows agree within the
  sum of their bounds over six steps;
* ``state_width``, the ``Optimizer`` / ``EvictRule`` validation,
  ``from_config``, and the CPU ``HostTable`` refusing the rule.
"""
import numpy as np
import pytest

import _ftrl_zn_oracle as Z
import _opt_oracle as O

STEPS = 6
SETTINGS = Z.settings()


def _optimizer(h, kind="ftrl_zn"):
    from swiftsnails_amd.ops.optim import Optimizer

    return Optimizer(**{**h.kwargs(), "kind": kind})


def _grads(g0, t):
    if t == 1:
        return g0
    if t % 2:
        return np.roll(g0, 5 * t)
    return np.random.default_rng(t).standard_normal(g0.shape).astype(np.float32)


@pytest.mark.parametrize("which", sorted(SETTINGS))
def test_fp32_evaluation_within_half_the_bound(which):
    h = SETTINGS[which]
    worst = 0.0
    for name, (z, n, g0) in (("planted", Z.planted(h)), ("gaussian", Z.gaussian(h, 4096, 3))):
        for t in range(1, STEPS + 1):
            g = _grads(g0, t)
            wref = Z.weight(h, O.as_n(z), O.as_n(n))
            wemu = Z.weight(h, O.as_n(z, np.float32), O.as_n(n, np.float32))
            ref, emu = Z.step(h, z, n, g), Z.step(h, z, n, g, T=np.float32)
            for i, (r, e) in enumerate(((wref, wemu), (ref[0], emu[0]), (ref[1], emu[1]))):
                assert e.v.dtype == np.float32
                rt = O.ratio(r, e.v, ftrl_w=i == 0)
                j = int(np.argmax(rt))
                assert rt[j] <= 0.5, (name, t, i, j, float(rt[j]), float(r.v[j]), float(e.v[j]))
                worst = max(worst, float(rt[j]))
            z, n = emu[0].v, emu[1].v
    print(f"CALIBRATION ftrl_zn {which} worst fp32/bound {worst:.3f}")


# the quantity each mutant is wrong in: the pulled weight, or z' of the step
CAUGHT_BY = {"zn_pull_is_z": "w", "zn_w_no_beta": "w", "zn_neg_zero": "w", "zn_no_sigma_w": "z"}


@pytest.mark.parametrize("which", sorted(SETTINGS))
@pytest.mark.parametrize("mutant", Z.MUTANTS)
def test_mutant_leaves_the_bound(mutant, which):
    """Every mutant leaves the bound on a planted coordinate of the quantity
    it is wrong in, under each of the three rule settings."""
    assert set(CAUGHT_BY) == set(Z.MUTANTS)
    h = SETTINGS[which]
    z, n, g = Z.planted(h)
    with np.errstate(invalid="ignore", divide="ignore"):
        if CAUGHT_BY[mutant] == "w":
            ref = Z.weight(h, O.as_n(z), O.as_n(n))
            mut = Z.weight(h, O.as_n(z, track=False), O.as_n(n, track=False), mutant)
            worst = float(O.ratio(ref, mut.v, ftrl_w=True).max())
        else:
            ref = Z.step(h, z, n, g)[0]
            mut = Z.step(h, z, n, g, mutant=mutant, track=False)[0]
            worst = float(O.ratio(ref, mut.v).max())
    assert worst > 1.0, (mutant, which, CAUGHT_BY[mutant], worst)


def test_planted_rows_hold_their_edges():
    for which in ("reg", "l1"):
        h = SETTINGS[which]
        z, n, g = Z.planted_threshold(h)
        assert (np.abs(z) <= np.float32(h.l1)).all()
        assert (Z.weight(h, O.as_n(z), O.as_n(n)).v == 0).all()
        z1 = Z.step(h, z, n, g)[0]
        # w = 0: z' = z + g' with nothing else in it
        np.testing.assert_array_equal(z1.v, z.astype(np.float64) + g.astype(np.float64) * h.grad_scale)
        on = np.abs(z1.v) == h.l1
        near = (np.abs(np.abs(z1.v) - h.l1) <= O.bound(z1)) & ~on
        assert on.sum() >= 4 and near.sum() >= 4
        assert ((np.abs(z1.v) > h.l1) & near).any() and ((np.abs(z1.v) < h.l1) & near).any()
    z, n, _ = Z.planted(SETTINGS["plain"])
    assert ((z == 0) & (n == 0)).any() and (n == 0).any() and (n >= 1e6).any()
    rows = Z.table_rows(SETTINGS["l1"], 700)
    assert rows.shape == (700, 2) and (np.abs(rows[:, 0]) <= np.float32(Z.L1)).any()
    assert (np.abs(rows[:, 0]) > np.float32(Z.L1)).any()


@pytest.mark.parametrize("which", sorted(SETTINGS))
def test_host_references_within_the_bound(which):
    from swiftsnails_amd.ops.optim import apply_reference, pull_reference

    h = SETTINGS[which]
    opt = _optimizer(h)
    rows = Z.table_rows(h, 700)
    worst = 0.0
    for s in range(STEPS):
        w = pull_reference(opt, rows, 1)
        assert w.shape == (len(rows), 1) and w.dtype == np.float32
        rp, ref = Z.pull_ratio(h, rows, w)
        assert rp.max() <= 1.0, ("pull", s, float(rp.max()), int(rp.argmax()))
        zero = np.abs(rows[:, 0]) <= np.float32(h.l1)
        assert zero.any() or s > 0   # the planted rows have them; with l1 = 0 they move off
        assert (w[zero, 0] == 0).all() and not np.signbit(w[zero, 0]).any()
        g = Z.table_grads(h, len(rows), s)
        after = apply_reference(opt, rows, g, 1)
        assert after.shape == rows.shape and after.dtype == np.float32
        ru = Z.rows_ratio(Z.step(h, rows[:, 0], rows[:, 1], g[:, 0]), after)
        assert ru.max() <= 1.0, ("step", s, float(ru.max()), np.unravel_index(ru.argmax(), ru.shape))
        worst = max(worst, float(rp.max()), float(ru.max()))
        rows = after
    print(f"CALIBRATION ftrl_zn {which} host references worst/bound {worst:.3f}")


@pytest.mark.parametrize("which", sorted(SETTINGS))
def test_same_trajectory_as_ftrl_from_zero(which):
    """From zero rows ``ftrl_zn`` and ``ftrl`` are one trajectory in exact
    arithmetic: the two fp32 host references, run freely for six steps on the
    same gradients, stay within the sum of the two oracles' running bounds."""
    from swiftsnails_amd.ops.optim import apply_reference, pull_reference

    h = SETTINGS[which]
    nk = 700
    a = np.zeros((nk, 2), np.float32)          # [z | n]
    b = np.zeros((nk, 3), np.float32)          # [w | z | n]
    oa = (O.as_n(a[:, 0]), O.as_n(a[:, 1]))
    ob = (O.as_n(b[:, 0]), O.as_n(b[:, 1]), O.as_n(b[:, 2]))
    ozn, oft = _optimizer(h), _optimizer(h, "ftrl")
    for s in range(STEPS):
        g = Z.table_grads(h, nk, s)
        a, b = apply_reference(ozn, a, g, 1), apply_reference(oft, b, g, 1)
        oa, ob = Z.step(h, *oa, g[:, 0]), O.step(h, *ob, g[:, 0])
        wa = Z.weight(h, *oa)
        for name, x, y, bx, by in (("z", a[:, 0], b[:, 1], oa[0], ob[1]),
                                   ("n", a[:, 1], b[:, 2], oa[1], ob[2]),
                                   ("w", pull_reference(ozn, a, 1)[:, 0], b[:, 0], wa, ob[0])):
            tol = O.bound(bx) + O.bound(by)
            d = np.abs(x.astype(np.float64) - y.astype(np.float64))
            assert (d <= tol).all(), (name, s, float((d / np.maximum(tol, 1e-300)).max()))
            # and the two oracles are one trajectory
            np.testing.assert_allclose(bx.v, by.v, rtol=1e-12, atol=1e-15)
    assert (b[:, 0] != 0).any()


def test_state_width_and_validation():
    from swiftsnails_amd.ops.optim import OPT_KINDS, EvictRule, Optimizer, state_width

    assert OPT_KINDS["ftrl_zn"] == 4
    assert state_width("ftrl_zn", 1) == 1 and Optimizer("ftrl_zn").state_width(1) == 1
    assert state_width("ftrl", 1) == 2 and state_width("adagrad", 1) == 1   # unchanged
    for bad in (dict(ftrl_alpha=0.0), dict(ftrl_alpha=-1.0), dict(l1=-0.1), dict(l2=-0.1),
                dict(ftrl_beta=-1.0)):
        with pytest.raises(ValueError, match="ftrl_zn"):
            Optimizer("ftrl_zn", **bad)
    with pytest.raises(ValueError, match="unknown optimizer"):
        Optimizer("ftrl_nz")
    opt = Optimizer("ftrl_zn", l1=0.3)
    assert EvictRule(w_below=0.0).native_args(opt) == (1, 0.0, 0, 0.0)
    assert EvictRule(acc_below=0.5).native_args(opt) == (0, 0.0, 1, 0.5)   # reads n
    with pytest.raises(ValueError):
        EvictRule().native_args(opt)


def test_from_config():
    from swiftsnails_amd.ops.optim import Optimizer

    o = Optimizer.from_config({"optimizer": "ftrl_zn", "l1": "0.3", "l2": "0.01",
                               "ftrl_alpha": "0.1", "ftrl_beta": "2"})
    assert (o.kind, o.l1, o.l2, o.ftrl_alpha, o.ftrl_beta) == ("ftrl_zn", 0.3, 0.01, 0.1, 2.0)
    d = Optimizer.from_config({"optimizer": "ftrl_zn"})
    assert (d.ftrl_alpha, d.ftrl_beta) == (0.05, 1.0)


def test_host_table_refuses_the_rule():
    from swiftsnails_amd._native import host
    from swiftsnails_amd.ops.host_table import HostTable
    from swiftsnails_amd.ops.optim import Optimizer

    with pytest.raises(ValueError, match="ftrl_zn"):
        HostTable(1, optimizer=Optimizer("ftrl_zn"))
    # ... and the native table itself, whoever builds its parameters
    h = host()
    with pytest.raises(Exception, match="ftrl_zn"):
        h.HostTable(1, 2, h.InitParams(0, 0.0, 0.0, 0, -1),
                    h.OptParams(4, 0.05, 0.0, 0.0, 1e-8, 0.9, 0.999, 1.0, 1.0, 0.05, 1.0, 1.0, 0.0),
                    1)
