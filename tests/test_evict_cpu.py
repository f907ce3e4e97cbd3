"""Eviction on the CPU table (``HostTable.evict`` / ``remove``, the rule of
``csrc/include/ss/evict.h``) against NumPy, and the preconditions of the
evicting fp64 oracle (``_evict_oracle.py``) that ``test_gpu_evict.py`` holds
the engine to — checked here from the oracle alone, on a machine without a
GPU.

Measured (the oracle's preconditions; asserted below, not tuned):

    binary32           5415 of 11847 keys evicted,  877 reappear, margin 29.1
    valued64           6638 of 11894 keys evicted, 1275 reappear, margin  7.5
    valued64, world 2  6640 of 11802 keys evicted, 1277 reappear, margin  9.6
"""
import numpy as np
import pytest
import torch

import _evict_oracle as E
import _lr_oracle as O

DIM, N = 3, 6000


def _table(kind):
    from swiftsnails_amd.ops.host_table import HostTable
    from swiftsnails_amd.ops.optim import InitConfig, Optimizer

    opt = Optimizer(kind, lr=0.1, l1=0.05 if kind == "ftrl" else 0.0)
    return HostTable(DIM, shard_num=4, optimizer=opt, init=InitConfig("uniform", 0.02, seed=11))


def _fill(t, seed=0):
    """N keys pulled, random subsets pushed a few times (so the accumulators
    differ), a sixth never pushed.  Returns (keys u64 sorted, rows) as stored."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(1, 1 << 50, N, dtype=np.int64))
    t.pull_keys(keys)
    pushed = keys[: len(keys) * 5 // 6]
    for r in range(4):
        sub = pushed[rng.random(len(pushed)) < 0.6]
        g = (rng.standard_normal((len(sub), DIM)) * rng.choice([0.01, 0.1, 1.0], (len(sub), 1)))
        t.push_keys(sub, g.astype(np.float32))
    return _export(t)


def _export(t):
    ks, rs = [], []
    for k, r in t.export():
        ks.append(k.numpy().view(np.uint64))
        rs.append(r.numpy())
    if not ks:
        return np.empty(0, np.uint64), np.empty((0, t.width), np.float32)
    k, r = np.concatenate(ks), np.concatenate(rs)
    o = np.argsort(k)
    return k[o], r[o]


def _acc(kind, rows):
    """The sum-of-squares block: AdaGrad s1, FTRL n (the second state block)."""
    off = {"adagrad": DIM, "ftrl": 2 * DIM}[kind]
    return rows[:, off:off + DIM]


def _check_evicted(t, keys, rows, victim, n):
    from swiftsnails_amd.ops.optim import init_reference

    assert 0 < victim.sum() < len(keys)  # the case has both kinds of key
    assert n == int(victim.sum()) and t.size() == len(keys) - n
    k2, r2 = _export(t)
    assert np.array_equal(k2, keys[~victim])
    assert np.array_equal(r2.view(np.uint32), rows[~victim].view(np.uint32))  # bit-identical
    _, found = t._t.get_rows(keys)
    assert np.array_equal(found.astype(bool), ~victim)
    # a victim pulled again restarts from its initial row
    t.pull_keys(keys[victim])
    back, found = t._t.get_rows(keys[victim])
    assert found.all() and t.size() == len(keys)
    assert np.array_equal(back, init_reference(t.init_cfg, keys[victim], DIM, t.width))


@pytest.mark.parametrize("kind", ["adagrad", "ftrl"])
def test_host_evict_acc_below_matches_numpy(kind):
    from swiftsnails_amd.ops.optim import EvictRule

    t = _table(kind)
    keys, rows = _fill(t)
    acc = _acc(kind, rows).max(1)
    thr = np.float32(np.median(acc))
    victim = acc <= thr
    _check_evicted(t, keys, rows, victim, t.evict(EvictRule(acc_below=float(thr))))


@pytest.mark.parametrize("kind", ["sgd", "adagrad", "ftrl"])
def test_host_evict_w_below_matches_numpy(kind):
    from swiftsnails_amd.ops.optim import EvictRule

    t = _table(kind)
    keys, rows = _fill(t, seed=1)
    wmax = np.abs(rows[:, :DIM]).max(1)
    thr = np.float32(np.median(wmax))
    victim = wmax <= thr
    _check_evicted(t, keys, rows, victim, t.evict(EvictRule(w_below=float(thr))))


def test_host_evict_both_conditions_and_nan_row_survives():
    from swiftsnails_amd.ops.optim import EvictRule

    t = _table("adagrad")
    keys, rows = _fill(t, seed=2)
    # a row with a NaN coordinate is a survivor under any threshold
    nan_row = rows[7].copy()
    nan_row[1] = np.float32("nan")
    t.assign(keys[7:8], nan_row[None])
    rows[7] = nan_row
    wmax, acc = np.abs(rows[:, :DIM]).max(1), _acc("adagrad", rows).max(1)
    tw, ta = np.float32(np.nanquantile(wmax, 0.7)), np.float32(np.quantile(acc, 0.6))
    with np.errstate(invalid="ignore"):
        victim = (wmax <= tw) & (acc <= ta)
    assert not victim[7]
    n = t.evict(EvictRule(w_below=float(tw), acc_below=float(ta)))
    assert n == int(victim.sum()) and 0 < n < len(keys)
    k2, r2 = _export(t)
    assert np.array_equal(k2, keys[~victim])
    assert np.array_equal(r2.view(np.uint32), rows[~victim].view(np.uint32))
    assert t.evict(EvictRule(w_below=float("inf"))) == len(keys) - n - 1  # all but the NaN row
    assert np.array_equal(_export(t)[0], keys[7:8])


def test_host_remove_keys_ignores_absent():
    t = _table("adagrad")
    keys, rows = _fill(t, seed=3)
    gone = keys[::3]
    absent = np.arange(1, 50, dtype=np.uint64) + np.uint64(1 << 55)
    n = t.remove(np.concatenate([gone, absent, gone[:10]]))
    victim = np.isin(keys, gone)
    _check_evicted(t, keys, rows, victim, n)
    assert t.remove(absent) == 0 and t.size() == len(keys)
    assert t.remove(torch.from_numpy(keys.view(np.int64))) == len(keys) and t.size() == 0


def test_rule_errors():
    from swiftsnails_amd.ops.optim import EvictRule

    t = _table("sgd")
    _fill(t, seed=4)
    with pytest.raises(ValueError):
        t.evict(EvictRule(acc_below=1.0))  # SGD rows have no sum-of-squares block
    with pytest.raises(ValueError):
        t.evict(EvictRule())
    with pytest.raises(ValueError):
        t.evict()
    assert t.size() > 0


def test_cpu_engine_evict():
    """PSEngine.evict on the CPU engine path: the shard's count, the table
    smaller, training goes on."""
    from swiftsnails_amd.ops.host_table import HostTable
    from swiftsnails_amd.ops.optim import EvictRule, InitConfig, Optimizer
    from swiftsnails_amd.parallel.engine import PSEngine

    t = HostTable(1, shard_num=2, optimizer=Optimizer("adagrad", lr=0.1), init=InitConfig("zero"))
    eng = PSEngine(t, None, max_keys=4096, dim=1, device="cpu")
    keys = torch.arange(1, 3001, dtype=torch.int64)
    rnd = eng.pull(keys)
    g = torch.where(keys % 2 == 0, 1.0, 1e-3).reshape(-1, 1)
    eng.accumulate(rnd, g)
    eng.push(rnd)
    assert t.size() == 3000
    assert eng.evict(EvictRule(acc_below=1e-4)) == 1500 and t.size() == 1500
    rnd = eng.pull(keys)  # the evicted keys come back as new keys
    eng.accumulate(rnd, g)
    eng.push(rnd)
    assert t.size() == 3000
    with pytest.raises(ValueError):
        eng.evict()


# ---------------------------------------------------------- the evicting oracle
@pytest.mark.parametrize("name,world", [("binary32", 1), ("valued64", 1), ("valued64", 2)])
def test_evicting_oracle_preconditions(name, world):
    ev = E.evicting_reference(name, world)
    print(f"EVICT ORACLE {name} world {world}: thr {ev.thr:.6g}, {len(ev.evicted)} of "
          f"{ev.n_before} evicted, {ev.reappear} reappear, margin {ev.margin:.1f}, "
          f"ill {ev.res.ill}")
    assert ev.margin >= 4            # no key's h is near the threshold
    assert ev.reappear >= 100        # evicted keys do come back in steps 4..7
    assert ev.res.ill == 0           # the oracle's own precondition
    assert 0.4 * ev.n_before <= len(ev.evicted) <= 0.6 * ev.n_before
    assert len(ev.res.losses) == O.STEPS
    # a key evicted and not seen again is gone; one seen again is back
    later = np.unique(np.concatenate([k.reshape(-1) for k, _, _ in
                                      O.batches(name, world)[E.EVICT_AFTER:]]))
    assert np.array_equal(np.isin(ev.evicted, ev.res.keys), np.isin(ev.evicted, later))
