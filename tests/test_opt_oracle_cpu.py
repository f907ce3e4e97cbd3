"""The update-rule oracle (``_opt_oracle.py``) held to itself and the host
table held to it, on the CPU.

* the oracle's fp32 evaluation stays within half its bound on every planted
  and Gaussian coordinate, every rule, plain and regularised, six steps taken
  one at a time from the fp32 rows;
* every planted mutant leaves the bound on a planted coordinate;
* ``HostTable`` (``opt_apply`` compiled for the host), four rules, dims 1 / 3
  / 8, six rounds of ``push_keys`` + ``next_round``: every step from the
  table's own rows, and for SGD and Adam the free-running fp64 trajectory from
  the initial rows — the Adam one pins the round counter (it fails at round 2
  when the corrections use ``t = max(1, step)``);
* an Adam table saved after three rounds and restored continues with the
  oracle's rounds 4-6; one left at ``step = 0`` does not.
"""
import numpy as np
import pytest

import _opt_oracle as O

STEPS = 6
CASES = sorted(O.SETTINGS)


def _optimizer(h):
    from swiftsnails_amd.ops.optim import Optimizer

    return Optimizer(**h.kwargs())


def _rows(table, keys):
    d = table.to_dict(with_state=True)
    return np.stack([d[int(k)] for k in keys.view(np.uint64)])


@pytest.mark.parametrize("kind,which", CASES)
def test_fp32_evaluation_within_half_the_bound(kind, which):
    h = O.setting(kind, which)
    worst = 0.0
    for name, (w, s1, s2, g0) in (("planted", O.planted(h)), ("gaussian", O.gaussian(h, 4096, 3))):
        rows = (w, s1, s2)
        for t in range(1, STEPS + 1):
            if t == 1:
                g = g0
            elif t % 2:
                g = np.roll(g0, 5 * t)
            else:
                g = np.random.default_rng(t).standard_normal(g0.shape).astype(np.float32)
            ref = O.step(h, *rows, g, t)
            emu = O.step(h, *rows, g, t, T=np.float32)
            for i, (r, e) in enumerate(zip(ref, emu)):
                if r is None:
                    continue
                assert e.v.dtype == np.float32
                rt = O.ratio(r, e.v, ftrl_w=kind == "ftrl" and i == 0)
                j = int(np.argmax(rt))
                assert rt[j] <= 0.5, (name, t, i, j, float(rt[j]), float(r.v[j]), float(e.v[j]))
                worst = max(worst, float(rt[j]))
            rows = tuple(None if e is None else e.v for e in emu)
    print(f"CALIBRATION {kind} {which} worst fp32/bound {worst:.3f}")


@pytest.mark.parametrize("mutant,kind", [(m, k) for m, ks in O.MUTANTS.items() for k in ks])
def test_mutant_leaves_the_bound(mutant, kind):
    h = O.setting(kind, "reg")
    w, s1, s2, g = O.planted(h)
    worst = 0.0
    for t in (1, 2, 3):
        ref = O.step(h, w, s1, s2, g, t)
        mut = O.step(h, w, s1, s2, g, t, mutant=mutant)
        for i, (r, m) in enumerate(zip(ref, mut)):
            if r is not None:
                worst = max(worst, float(O.ratio(r, m.v, ftrl_w=kind == "ftrl" and i == 0).max()))
    assert worst > 1.0, (mutant, kind, worst)


def test_planted_inputs_hold_their_edges():
    h = O.setting("ftrl", "reg")
    g = O.planted_grads(h).astype(np.float64) * h.grad_scale
    assert (g == h.clip).any() and (g == -h.clip).any() and (g == 0).any()
    assert ((g > 0) & (g < h.clip) & (g > h.clip * (1 - 2.0 ** -22))).any()   # one ulp inside
    raw = np.abs(O.planted_grads(h))
    assert (np.abs(g) > 30 * h.clip).any()                         # well outside
    assert (raw == np.float32(1e-12)).any() and (raw == np.float32(1e4)).any()
    w, z, n, gt = O.planted_threshold(h)
    z1 = O.step(h, w, z, n, gt)[1]
    on = np.abs(z1.v) == h.l1
    near = (np.abs(np.abs(z1.v) - h.l1) <= O.bound(z1)) & ~on
    assert on.sum() >= 4 and near.sum() >= 4 and (np.abs(np.abs(z1.v) - h.l1) > 0.5).any()
    assert ((np.abs(z1.v) > h.l1) & near).any() and ((np.abs(z1.v) < h.l1) & near).any()
    assert (O.planted_states(h)[2] == 0).any()                     # first touch
    assert (O.planted_states(O.setting("adagrad", "reg"))[1] == np.float32(0.05)).any()
    _, m, v = O.planted_states(O.setting("adam", "reg"))
    assert ((m == 0) & (v == 0)).any() and ((v > 0) & (np.sqrt(v) < 0.2 * h.eps)).any()


def test_bf16_interval():
    x = np.array([1.0, 1.0 + 2.0 ** -9, -1.0 - 2.0 ** -9, 0.0, 3.0e-5, -7.7])
    lo, hi = O.bf16_interval(x, x)
    assert (lo <= x).all() and (hi >= x).all()
    for a in (lo, hi):
        assert ((a.view(np.uint32) & 0xFFFF) == 0).all()
    assert lo[0] == hi[0] == 1.0 and lo[3] == hi[3] == 0.0
    assert lo[1] == 1.0 and hi[1] == np.float32(1.0 + 2.0 ** -7)
    assert hi[2] == -1.0 and lo[2] == np.float32(-1.0 - 2.0 ** -7)


def _host_run(h, dim, opt=None, nkeys=257, steps=STEPS, table=None, first=0):
    """Six rounds through a HostTable; per round the rows before, the
    gradients and the rows after."""
    from swiftsnails_amd.ops.host_table import HostTable

    keys = (np.arange(nkeys, dtype=np.int64) * 7919 + 11) << 20
    if table is None:
        table = HostTable(dim, shard_num=3, optimizer=opt or _optimizer(h))
        table.assign(keys, O.table_rows(h, nkeys, dim))
    out = []
    for s in range(first, first + steps):
        before = _rows(table, keys)
        g = O.table_grads(h, nkeys, dim, s)
        table.push_keys(keys, g)
        table.next_round()
        out.append((before, g, _rows(table, keys)))
    return table, keys, out


@pytest.mark.parametrize("dim", [1, 3, 8])
@pytest.mark.parametrize("kind,which", CASES)
def test_host_table_matches_oracle(kind, which, dim):
    h = O.setting(kind, which)
    _, _, rounds = _host_run(h, dim)
    free = O.split(kind, rounds[0][0], dim)
    worst = 0.0
    for t, (before, g, after) in enumerate(rounds, 1):
        _, _, parts = O.step_rows(h, before, g, dim, t)
        r = O.rows_ratio(h, parts, after, dim)
        assert r.max() <= 1.0, ("step", t, float(r.max()), np.unravel_index(r.argmax(), r.shape))
        worst = max(worst, float(r.max()))
        if kind in ("sgd", "adam"):
            free = O.step(h, *free, g, t)
            r = O.rows_ratio(h, free, after, dim)
            assert r.max() <= 1.0, ("free-running", t, float(r.max()))
    print(f"MARGIN host {kind} {which} dim {dim}: {worst:.3f}")


def test_free_running_adam_rejects_a_lagging_counter():
    """The parent's counter (corrections from t = max(1, step), the step
    advanced after the push) gives rounds t = 1, 1, 2, ...: the free-running
    check must fail at round 2, so it is known to pin the counter."""
    h = O.setting("adam", "plain")
    from swiftsnails_amd.ops.optim import Optimizer

    class Lagging(Optimizer):
        def bias_corrections(self):
            t = max(1, self.step)
            return 1.0 / (1.0 - self.beta1 ** t), 1.0 / (1.0 - self.beta2 ** t)

    lag = Lagging(**h.kwargs())
    _, _, rounds = _host_run(h, 3, opt=lag)
    free = O.split("adam", rounds[0][0], 3)
    failed = None
    for t, (_, g, after) in enumerate(rounds, 1):
        free = O.step(h, *free, g, t)
        if failed is None and O.rows_ratio(h, free, after, 3).max() > 1.0:
            failed = t
    assert failed == 2


@pytest.mark.parametrize("fmt", ["bin", "text"])
def test_adam_checkpoint_continues_the_rounds(tmp_path, fmt):
    from swiftsnails_amd.ops.host_table import HostTable
    from swiftsnails_amd.utils import checkpoint as ck

    h, dim = O.setting("adam", "reg"), 3
    t, keys, rounds = _host_run(h, dim, steps=3)
    assert t.opt.step == 3
    p = str(tmp_path / f"adam.{fmt}")
    if fmt == "bin":
        ck.save_binary(t, p)
    else:
        ck.save_text(t, p, with_state=True)
    free = O.split("adam", rounds[0][0], dim)
    for s, (_, g, _) in enumerate(rounds, 1):
        free = O.step(h, *free, g, s)

    def resume(step):
        t2 = HostTable(dim, shard_num=5, optimizer=_optimizer(h))
        (ck.load_binary if fmt == "bin" else ck.load_text)(t2, p)
        if step is not None:
            t2.opt.step = step
        _, _, more = _host_run(h, dim, table=t2, first=3, steps=3)
        f, worst = free, []
        for s, (before, g, after) in enumerate(more, 4):
            r1 = O.rows_ratio(h, O.step_rows(h, before, g, dim, s)[2], after, dim).max()
            f = O.step(h, *f, g, s)
            worst.append(max(float(r1), float(O.rows_ratio(h, f, after, dim).max())))
        return t2, worst

    if fmt == "bin":   # the binary header carries opt_step
        t2, worst = resume(None)
        assert t2.opt.step == 6 and max(worst) <= 1.0, worst
    else:              # text has no header: the caller restores the counter
        t2, worst = resume(3)
        assert max(worst) <= 1.0, worst
    _, worst0 = resume(0)  # a counter left at 0 must not pass: the check bites
    assert min(worst0) > 1.0, worst0


def test_local_train_client_counts_adam_rounds():
    """``local_train`` (an in-process HostTable behind the worker API): each
    push is a round, so three Adam pushes follow the oracle's t = 1, 2, 3."""
    from swiftsnails_amd.framework.cluster import _LocalClient, _cfg

    c = _LocalClient(_cfg({"optimizer": "adam", "learning_rate": 0.01, "local_train": 1}), 2)
    h = O.Hyper("adam", lr=0.01).f32()
    keys = np.arange(1, 40, dtype=np.uint64)
    free = (np.zeros((len(keys), 2), np.float32),) * 3
    for t in (1, 2, 3):
        g = O.table_grads(h, len(keys), 2, t)
        c.push(keys, g)
        free = O.step(h, *free, g, t)
    got = _rows(c.table, keys.view(np.int64))
    assert O.rows_ratio(h, free, got, 2).max() <= 1.0


# ------------------------------------------- the engine cases' preconditions
ENGINE_CASES = [("ftrl_l1", "valued64", 1), ("ftrl_l1", "binary32", 1), ("ftrl_l1", "valued64", 2),
                ("adam", "binary32", 1), ("adam", "valued64", 2),
                ("adagrad_l2_clip", "valued64", 1), ("adagrad_l2_clip", "binary32", 1),
                ("sgd_l2", "valued64", 1)]


@pytest.mark.parametrize("tag,name,world", ENGINE_CASES)
def test_lr_oracle_new_rules_precondition_and_noise_floor(tag, name, world):
    """What ``test_gpu_opt_oracle.py``'s engine cases rely on, from the oracle
    alone: no ill-conditioned key-step, the same model in fp32 with permuted
    sums within half the tolerance, and for FTRL under 1 % of the keys with
    ``|z| - l1`` inside z's tolerance and the zero set equal outside them."""
    import _lr_oracle as L

    opt, reg = L.OPT_SETTINGS[tag]
    ref = L.opt_reference(tag, name, world)
    assert ref.ill == 0 and np.isfinite(ref.tol_w).all() and np.isfinite(ref.tol_h).all()
    f = L.run(name, opt, world, L.OPT_STEPS, dtype=np.float32, perm=5, **dict(reg))
    two = opt in ("ftrl", "adam")
    rw, rh, out = L.ratios(ref, f.keys, f.w, f.h if opt != "sgd" else None, f.h2 if two else None)
    print(f"CALIBRATION lr {tag} {name} world {world}: fp32 / tol  w {rw:.3f}  state {rh:.3f}")
    assert rw <= 0.5 and rh <= 0.5 and out == 0
    if opt == "ftrl":
        near = L.ftrl_near_threshold(ref, dict(reg)["l1"])
        assert near.mean() < 0.01 and 0.05 < (ref.w == 0).mean() < 0.5
        assert np.array_equal((ref.w == 0)[~near], (f.w == 0)[~near])
