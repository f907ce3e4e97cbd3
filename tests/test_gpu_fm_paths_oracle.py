"""The factorization machine through every path it trains on, against the fp64
oracle of ``_fm_oracle.py``.

Every case trains eight synchronous rounds (``SS_PULL_AHEAD=0``) from an
HBM-resident ``FileCtrSource`` whose batches are checked bit for bit against
the arrays the oracle steps on, and is held to the oracle **step by step**
(``_fm_oracle.Stepwise``): the table is exported after every round, the
oracle computes that round in fp64 from the table's own rows before it, and
every coordinate of every key's parameters and AdaGrad state must sit within
that round's tolerance; keys the batch did not touch must be bit-identical.
(A carried bound over eight free-running AdaGrad rounds cannot hold even the
reference's own fp32 evaluation; ``_fm_oracle.py`` says why.  SGD has no
denominator: its cases are also held to the free-running reference at the
end, ``MARGIN ... free-running``.)  Asserted in every case: the oracle's
precondition (no ill-conditioned key-step, from the oracle alone and again on
the engine's own trajectory), each step's mean loss (rtol 1e-4), the exported
key set (exactly the oracle's: no EMPTY key, one slot per key), every
coordinate, and what ran (``w.bucketed``, ``eng.fast1``, ``eng.xg``).

**Open defect.**  Every case runs in a spawned process of its own
(``_fresh``).  Run inside the one pytest process, as ``test_gpu_lr_paths_
oracle.py`` runs, this module made a later, unrelated test fail in four of
five whole-suite runs: ``test_gpu_models.py::test_graph_teardown_then_replay_
same_process`` — the start-up litmus of its size-1 xGMI arena read wrong
words (once 5120; once the same 1888 words of part 0 of the ``keys`` mailbox
in every round, on both tiers), or its graph replays ended in a NaN loss.
The same order without this module passed twice; single runs without its
pull-ahead cases, or without its world-1 xGMI cases, passed; a run without
its child-process cases failed.  So something an engine or an arena of these
cases leaves on the device or in the process reaches a later arena or graph,
although ``conftest.py`` collects garbage and synchronises after every GPU
test.  The cause is not found; the isolation keeps the suite reliable and
fixes nothing in the engine or the transport (``docs/TESTING.md``).

New keys start from the device's initialiser: the oracle takes their rows
from a scratch table with the same ``InitConfig`` (the initialiser is a
function of key and column alone), and ``test_device_init_within_the_
relative_term`` measures the host mirror against it.

Cases: the fast path at ``dim`` 2 / 5 / 9 / 17 (17: the scalar and
two-column-pass branches) and with SGD; ``fm_hot`` (the overflow list and the
LDS-atomic merge; ``worker.ovf[0] >= 1`` asserted) with SGD and AdaGrad; the
row-atomic fallback, by dedup mode and by width (``fm_narrow``); the xGMI
unique exchange at world 1 and world 2 (the union-batch oracle); bf16 rows;
``SS_FM_REDUCE=atomic`` in a spawned child (read once per process); and
pull-ahead as shipped (staleness 1, ``SS_PULL_STREAM`` 0 and 1) as a replay:
each round's gradient is computed from the rows the engine actually pulled,
every pulled coordinate must be bit-identical to the table after push i-2 or
after push i-1, and the table after every push must match the replay.

Measured on an MI355X, the largest |engine - oracle| / tol per path (x, h;
each case prints its own as ``MARGIN ...``; reported, not tuned):

    fast path, dim 2 / 5 / 9 / 17    0.041 / 0.081 / 0.068 / 0.044   h 0.024-0.028
    fast path, SGD                   0.001   (free-running 0.012)
    overflow (fm_hot), SGD 9 / 17    0.001   (free-running 0.014)
    overflow (fm_hot), AdaGrad       0.031 / 0.052                   h 0.029 / 0.034
    fallback, hash dedup 9 / 17      0.068 / 0.056                   h 0.041 / 0.026
    fallback by width (fm_narrow)    0.058                           h 0.031
    xGMI unique, world 1             0.068, SGD 0.001 (0.012)        h 0.026
    xGMI unique, world 2             0.068, SGD 0.001 (0.012)        h 0.024
    SS_FM_REDUCE=atomic              0.068                           h 0.026
    pull-ahead replay, both streams  0.068                           h 0.026
    bf16 rows, / (0.02 + 0.03 |ref|) 0.226

The fp32 NumPy evaluation of the model sits at 0.04-0.10 (x) and 0.03-0.04
(h): every path is at the model's own fp32 noise floor.  The device's
initialiser is within 1.9e-8 of its host mirror (0.015 of ``1e-6 + 1e-4
|x|``).  Pull-ahead: of the 263682 pulled coordinates that push i-1 changed,
none held the newer value with either stream — at this size every pulled
round read the table exactly one push stale, which is legal, and every push
matched the replay: the merges are right under pull-ahead, so a loss that
differs from the synchronous run's is staleness, not a wrong merge.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _fm_oracle as O
from _lr_oracle import B, EMPTY, STEPS
from _mp import collect, file_init, init_gloo, in_child

pytestmark = pytest.mark.gpu

CAP = 1 << 18
KNOBS = ("SS_CLAIM", "SS_SLOT32", "SS_TABLE_REGIONS", "SS_ENGINE_GENERAL", "SS_DEDUP",
         "SS_SRV_STAGE", "SS_XGMI_SELF", "SS_SERVER_STREAM", "SS_STALENESS", "SS_ENGINE_DEPTH",
         "SS_TABLE_G", "SS_FM_REDUCE", "SS_PULL_STREAM")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("fm_oracle")
    return {n: O.dataset(n).write(d / f"{n}.libsvm") for n in O.F}


def _table(optimizer, dim, dev, lr=None, row_dtype="fp32"):
    from swiftsnails_amd.models.fm import fm_table_args
    from swiftsnails_amd.ops.optim import Optimizer
    from swiftsnails_amd.ops.table import HbmTable

    opt, init = fm_table_args(dim - 1, Optimizer(optimizer, lr=lr or O.LR[optimizer], eps=O.EPS))
    assert (init.kind, init.scale, init.state_init) == ("normal", O.INIT_SCALE, 0.0)
    return HbmTable(dim, CAP, optimizer=opt, init=init, device=dev, row_dtype=row_dtype)


_INIT = {}


def _init_rows(dev, dim):
    """keys -> the device's initial parameters [n, dim], read from a scratch
    table once per dim (every key of every data set)."""
    if dim not in _INIT:
        keys = np.unique(np.concatenate([O.dataset(n).keys.reshape(-1) for n in O.F]))
        keys = keys[keys != EMPTY]
        t = _table("sgd", dim, dev)
        rows, _ = t.pull(torch.from_numpy(keys.view(np.int64)).to(dev))
        torch.cuda.synchronize()
        t.check()
        _INIT[dim] = (keys, rows.cpu().numpy())
    keys, rows = _INIT[dim]

    def f(k):
        pos = np.searchsorted(keys, k)
        assert np.array_equal(keys[pos], k)
        return rows[pos]
    return f


def _source(path, name, batch, dev, rank=0, world=1):
    """The HBM-resident file source, its batches checked against the arrays
    the oracle steps on."""
    from swiftsnails_amd.utils.dataio import FileCtrSource

    ds, nf = O.dataset(name), O.F[name]
    src = FileCtrSource(path, batch_size=batch, num_fields=nf, rank=rank, world=world,
                        resident="hbm", device=dev)
    lo, hi = ds.shard(rank, world)
    assert src.rows == hi - lo and not src.has_values
    k = torch.empty(batch * nf, dtype=torch.int64, device=dev)
    y = torch.empty(batch, dtype=torch.float32, device=dev)
    for t in range(STEPS):
        src.generate(t, rank, world, k, y)
        ek, _, ey = ds.batch(t, batch, rank, world)
        assert np.array_equal(k.cpu().numpy().view(np.uint64), ek.reshape(-1)), t
        assert np.array_equal(y.cpu().numpy(), ey), t
    return src


def _engine(path, table, dev, monkeypatch, name, dedup=None, pull_ahead="0"):
    """The engine of 'fast' or 'unique' at world 1 (knobs set before it is built)."""
    from swiftsnails_amd.parallel.engine import PSEngine
    from swiftsnails_amd.parallel.xgmi import XgmiTransport

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if pull_ahead is None:
        monkeypatch.delenv("SS_PULL_AHEAD", raising=False)
    else:
        monkeypatch.setenv("SS_PULL_AHEAD", pull_ahead)
    monkeypatch.setenv("SS_XGMI_TIMEOUT", "30")
    if dedup:
        monkeypatch.setenv("SS_DEDUP", dedup)
    tr = None if path == "fast" else XgmiTransport(0, 1, dev, None, timeout_s=30)
    eng = PSEngine(table, tr, max_keys=B * O.F[name], dim=table.dim, device=dev)
    return eng, tr


def _export(table):
    ks, rs = [], []
    for k, r in table.export():
        ks.append(k.numpy())
        rs.append(r.numpy())
    return np.concatenate(ks).view(np.uint64), np.concatenate(rs)


def _split(rows, D, ada):
    return rows[:, :D], (rows[:, D:2 * D] if ada else None)


def _train_stepwise(w, table, sw, name, ada, each=None):
    """Eight rounds, the table held to the oracle after each (``each()``: a
    case's own per-round assertion); returns the engine's mean losses and the
    last export."""
    D, losses = table.dim, []
    for t, (bk, y) in enumerate(O.batches(name)):
        w.step()
        losses.append(w.mean_loss())
        torch.cuda.synchronize()
        if each is not None:
            each()
        keys, rows = _export(table)
        assert EMPTY not in keys and len(np.unique(keys)) == len(keys)  # one slot per key
        sw.step(bk, y, keys, *_split(rows, D, ada))
    return losses, keys, rows


def _check(label, sw, losses, world=1):
    """The assertions of every case; prints the margin before asserting it."""
    assert sw.ill == 0  # no ill-conditioned key-step on the engine's own trajectory either
    want = np.array([l.reshape(world, -1).mean(1) for l in sw.losses])
    for r, l in enumerate(losses):
        np.testing.assert_allclose(l, want[:, r], rtol=1e-4)
    print(f"MARGIN {label}: max |engine - oracle| / tol  x {sw.rx:.3f}  h {sw.rh:.3f}")
    assert sw.rx <= 1 and sw.rh <= 1, (label, sw.rx, sw.rh, sw.out)


def _check_free_running(label, ref, keys, x):
    """SGD: the final table against the free-running reference too."""
    assert ref.ill == 0
    rx, _, out = O.ratios(ref, keys, x)
    print(f"MARGIN {label} free-running: max |engine - oracle| / tol  x {rx:.3f}")
    assert rx <= 1, (label, rx, out)


def _body_device_init_within_the_relative_term():
    """The host mirror of the normal initialiser against the device's, every
    key of every data set, 17 columns: inside a quarter of the tolerance's
    data-independent terms (the oracle itself starts from the device's rows)."""
    dev, monkeypatch = _child_env()
    from swiftsnails_amd.ops.optim import InitConfig, init_reference

    _init_rows(dev, 17)
    keys, rows = _INIT[17]
    ref = init_reference(InitConfig("normal", O.INIT_SCALE, 0.0), keys, 17, 17)
    diff = np.abs(rows.astype(np.float64) - ref)
    ratio = diff / (1e-6 + 1e-4 * np.abs(ref))
    print(f"MARGIN device init: max |device - host| {diff.max():.3e}, "
          f"/ (1e-6 + 1e-4 |x|) {ratio.max():.4f}, bit-identical {np.mean(rows == ref):.1%}")
    assert ratio.max() <= 0.25


def _run_world1(dev, files, monkeypatch, path, name, optimizer, dim, dedup=None):
    from swiftsnails_amd.models.fm import FMWorker

    lr = O.default_lr(name, optimizer)
    assert O.reference(name, optimizer, dim - 1).ill == 0  # the precondition, oracle alone
    table = _table(optimizer, dim, dev, lr)
    eng, tr = _engine(path, table, dev, monkeypatch, name, dedup)
    w = FMWorker(eng, _source(files[name], name, B, dev))
    assert not eng.pull_ahead
    sw = O.Stepwise(dim - 1, optimizer, lr, _init_rows(dev, dim))
    return table, eng, tr, w, sw


def _finish(label, table, eng, tr, w, sw, name, optimizer, dim, each=None):
    ada = optimizer == "adagrad"
    losses, keys, rows = _train_stepwise(w, table, sw, name, ada, each)
    eng.check()
    table.check()
    if tr is not None:
        tr.close()
    _check(label, sw, [losses])
    if not ada:
        _check_free_running(label, O.reference(name, optimizer, dim - 1), keys, rows[:, :dim])


def _body_fm_fast_path_matches_fp64_oracle(files, dim, optimizer):
    dev, monkeypatch = _child_env()
    name = "fm_spread"
    table, eng, tr, w, sw = _run_world1(dev, files, monkeypatch, "fast", name, optimizer, dim)
    assert w.bucketed and eng.fast1 and eng.xg is None
    _finish(f"fast {name} {optimizer} dim {dim}", table, eng, tr, w, sw, name, optimizer, dim)
    assert int(w.ovf[0]) == 0  # no bucket of this data set overflows


def _body_fm_overflow_bucket_matches_fp64_oracle(files, dim, optimizer):
    """``fm_hot``: the hot key's bucket goes to the overflow list and the
    LDS-atomic merge (``k_bd_reduce_fm<17>``: column groups of 8)."""
    dev, monkeypatch = _child_env()
    name = "fm_hot"
    table, eng, tr, w, sw = _run_world1(dev, files, monkeypatch, "fast", name, optimizer, dim)
    assert w.bucketed and eng.fast1 and eng.xg is None

    def overflowed():
        assert int(w.ovf[0]) >= 1  # the overflow path ran, in every round

    _finish(f"overflow {name} {optimizer} dim {dim}", table, eng, tr, w, sw, name, optimizer, dim,
            each=overflowed)


def _body_fm_row_atomic_fallback_matches_fp64_oracle(files, name, dim, dedup):
    """``fm_fwd_bwd`` with row atomics: by a non-bucket dedup mode, and chosen
    by ``FMWorker`` itself where the lane group (8 at F = 6) is below K = 16."""
    dev, monkeypatch = _child_env()
    table, eng, tr, w, sw = _run_world1(dev, files, monkeypatch, "fast", name, "adagrad", dim,
                                        dedup)
    assert not w.bucketed and eng.fast1
    assert all(dd.mode == ("hash" if dedup else "bucket") for dd in eng.dedupers)
    _finish(f"fallback {name} {dedup or 'by width'} dim {dim}", table, eng, tr, w, sw, name,
            "adagrad", dim)


def _body_fm_xgmi_unique_world1_matches_fp64_oracle(files, optimizer):
    """The N>1 path on a size-1 mailbox arena."""
    dev, monkeypatch = _child_env()
    name, dim = "fm_spread", 9
    table, eng, tr, w, sw = _run_world1(dev, files, monkeypatch, "unique", name, optimizer, dim)
    assert w.bucketed and not eng.fast1 and eng.xg is not None and not eng.records
    _finish(f"xgmi unique world 1 {optimizer}", table, eng, tr, w, sw, name, optimizer, dim)


def _body_fm_bf16_rows(files):
    """Compact bf16 rows (fp32 math, stochastically rounded updates): the
    oracle's key set exactly and, round by round from the table's own rows,
    every coordinate within the bounds ``test_records_own_bf16_rows`` uses
    (rtol 0.03, atol 0.02; a bf16 rounding is 2^-8 relative).  Held to the
    free-running reference instead, 0.52 % of the coordinates miss those
    bounds, by up to 0.136: a coordinate's first AdaGrad step is ``-lr
    sign(G)``, and bf16 noise in the other rows flips the sign of a small
    ``G_f`` (2 lr = 0.1 apart)."""
    dev, monkeypatch = _child_env()
    from swiftsnails_amd.models.fm import FMWorker

    name, dim = "fm_spread", 9
    assert O.reference(name, "adagrad", dim - 1).ill == 0
    table = _table("adagrad", dim, dev, row_dtype="bf16")
    eng, tr = _engine("fast", table, dev, monkeypatch, name)
    w = FMWorker(eng, _source(files[name], name, B, dev))
    assert w.bucketed and eng.fast1
    fp32_init = _init_rows(dev, dim)

    def init_rows(k):
        """A compact row holds its initial values rounded to bf16, to nearest even."""
        u = fp32_init(k).view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32)

    sw = O.Stepwise(dim - 1, "adagrad", O.LR["adagrad"], init_rows)
    losses, worst = [], 0.0
    for bk, y in O.batches(name):
        w.step()
        losses.append(w.mean_loss())
        torch.cuda.synchronize()
        keys, rows = _export(table)
        assert EMPTY not in keys and len(np.unique(keys)) == len(keys)
        sw.step(bk, y, keys, rows[:, :dim], rows[:, dim:2 * dim])  # the key set, untouched rows
        for got, ref in ((sw.x, sw.last.x), (sw.h, sw.last.h)):
            worst = max(worst, float((np.abs(got - ref) / (0.02 + 0.03 * np.abs(ref))).max()))
    eng.check()
    table.check()
    assert sw.ill == 0
    want = [l.mean() for l in sw.losses]
    np.testing.assert_allclose(losses, want, rtol=1e-4)
    assert losses[-1] < losses[0]
    print(f"MARGIN bf16 rows: max |engine - oracle| / (0.02 + 0.03 |ref|) {worst:.3f}")
    assert worst <= 1


# ---------------------------------------------------- SS_FM_REDUCE=atomic
def _atomic_body(path):
    """In a fresh process: the LDS-atomic merge for every bucket."""
    assert "swiftsnails_amd._native" not in sys.modules  # the knob is read once per process
    dev, env = _child_env()
    name, dim = "fm_spread", 9
    table, eng, tr, w, sw = _run_world1(dev, {name: path}, env, "fast", name, "adagrad", dim)
    os.environ["SS_FM_REDUCE"] = "atomic"  # read at the first merge launch
    assert w.bucketed and eng.fast1
    # only the sorted merge touches the overflow list (it zeroes the count at
    # every launch): a sentinel there must survive all eight rounds
    w.ovf[0] = -1

    def untouched():
        assert int(w.ovf[0]) == -1

    _finish("SS_FM_REDUCE=atomic", table, eng, tr, w, sw, name, "adagrad", dim, each=untouched)


def test_fm_lds_atomic_merge_matches_fp64_oracle(files):
    in_child(_atomic_body, files["fm_spread"], always=True)


# ------------------------------------------------------------------ world 2
def _rank(rank, world, path, optimizer, init, q):
    os.environ["SS_PULL_AHEAD"] = "0"
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    for k in KNOBS:
        os.environ.pop(k, None)
    init_gloo(init, rank, world)
    try:
        from swiftsnails_amd.models.fm import FMWorker
        from swiftsnails_amd.parallel.engine import PSEngine
        from swiftsnails_amd.parallel.transport import TorchDistTransport
        from swiftsnails_amd.parallel.xgmi import XgmiTransport

        name, dim = "fm_spread", 9
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        tr = XgmiTransport(rank, world, dev, dist.distributed_c10d._get_default_store(),
                           aux=TorchDistTransport(), timeout_s=30)
        table = _table(optimizer, dim, dev)
        eng = PSEngine(table, tr, max_keys=B // world * O.F[name], dim=dim, device=dev)
        w = FMWorker(eng, _source(path, name, B // world, dev, rank, world), rank=rank,
                     world=world)
        flags = {"bucketed": bool(w.bucketed), "fast1": bool(eng.fast1), "xg": eng.xg is not None,
                 "records": bool(eng.records), "ahead": bool(eng.pull_ahead)}
        if rank == 0:  # the device's initial rows, for the parent's oracle
            _init_rows(dev, dim)
        losses, snaps = [], []
        for _ in range(STEPS):
            w.step()
            losses.append(w.mean_loss())
            torch.cuda.synchronize()
            dist.barrier()  # both ranks' pushes of this round are applied
            snaps.append(_export(table))
            dist.barrier()
        eng.check()
        table.check()
        q.put((rank, losses, snaps, flags, _INIT.get(dim)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_fm_world2_matches_fp64_oracle(files, optimizer):
    """Two ranks on one GPU, each reading its half of the file: a synchronous
    round is one update per key on the sum of both ranks' gradients, the
    world-1 update of the union batch."""
    world, name, dim = 2, "fm_spread", 9
    ada = optimizer == "adagrad"
    assert O.reference(name, optimizer, dim - 1, world).ill == 0
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    init = file_init()
    procs = [ctx.Process(target=_rank, args=(r, world, files[name], optimizer, init, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = collect(q, procs, world, 180)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort(key=lambda x: x[0])
    for _, _, _, f, _ in res:
        assert f["bucketed"] and not f["fast1"] and f["xg"] and not f["records"] and not f["ahead"]
    ikeys, irows = res[0][4]

    def init_rows(k):
        pos = np.searchsorted(ikeys, k)
        assert np.array_equal(ikeys[pos], k)
        return irows[pos]

    sw = O.Stepwise(dim - 1, optimizer, O.LR[optimizer], init_rows)
    for t, (bk, y) in enumerate(O.batches(name, world)):
        keys = np.concatenate([r[2][t][0] for r in res])
        rows = np.concatenate([r[2][t][1] for r in res])
        assert all(len(r[2][t][0]) > 0 for r in res)  # both shards hold keys
        assert EMPTY not in keys and len(np.unique(keys)) == len(keys)
        sw.step(bk, y, keys, *_split(rows, dim, ada))
    _check(f"world 2 xgmi unique {optimizer}", sw, [r[1] for r in res], world=world)
    if not ada:
        _check_free_running(f"world 2 xgmi unique {optimizer}",
                            O.reference(name, optimizer, dim - 1, world), keys, rows[:, :dim])


# --------------------------------------------------------------- pull-ahead
def _pulled_rows(rnd, bk, dim):
    """The rows a pulled round holds, by key: (sorted distinct keys of the
    batch, their rows), every occurrence of a key resolving to one row."""
    n = bk.size
    uid = rnd.dd.owner.unique_ids(n).cpu().numpy()
    flat = bk.reshape(-1)
    assert np.array_equal(uid >= 0, flat != EMPTY)
    u, first, inv = np.unique(flat[uid >= 0], return_index=True, return_inverse=True)
    ids = uid[uid >= 0]
    assert np.array_equal(ids, ids[first][inv]) and len(np.unique(ids[first])) == len(u)
    return u, rnd.uvals[torch.from_numpy(ids[first]).to(rnd.uvals.device)].cpu().numpy()[:, :dim]


def _body_fm_pull_ahead_replay_matches_fp64_oracle(files, pull_stream):
    """Pull-ahead as shipped.  The pull of round i is enqueued before push
    i-1 and waits only for push i-2, so each pulled coordinate may come from
    the table after push i-2 or after push i-1, never older and nothing else
    (bit for bit); the oracle replays every round from the rows actually
    pulled, and the table after every push must match the replay."""
    dev, monkeypatch = _child_env()
    from swiftsnails_amd.models.fm import FMWorker

    name, dim, K = "fm_spread", 9, 8
    assert O.reference(name, "adagrad", K).ill == 0
    table = _table("adagrad", dim, dev)
    eng, tr = _engine("fast", table, dev, monkeypatch, name, pull_ahead=None)
    monkeypatch.setenv("SS_PULL_STREAM", pull_stream)
    w = FMWorker(eng, _source(files[name], name, B, dev))
    assert w.bucketed and eng.fast1 and eng.pull_ahead and eng.staleness == 1
    assert (eng.pull_stream is not None) == (pull_stream == "1")
    init_rows = _init_rows(dev, dim)
    sw = O.Stepwise(K, "adagrad", O.LR["adagrad"], init_rows)
    batches = O.batches(name)
    older = (np.empty(0, np.uint64), np.empty((0, dim), np.float32))  # the table after push i-2
    newer = older                                                     # ... after push i-1
    pulled, losses, fresh, total = None, [], 0, 0

    def rows_at(state, u):
        """state's rows of keys u; keys it does not hold yet: the initial rows."""
        k, x = state
        out = init_rows(u).copy()
        if len(k):
            pos = np.searchsorted(k, u).clip(max=len(k) - 1)
            hit = k[pos] == u
            out[hit] = x[pos[hit]]
        return out

    for t, (bk, y) in enumerate(batches):
        if pulled is not None:  # rows recorded after the previous step: round t's pull
            u, p = pulled
            a, b = rows_at(older, u), rows_at(newer, u)
            ok = (p == a) | (p == b)
            assert ok.all(), (t, int((~ok).sum()))
            fresh += int(((p == b) & (p != a)).sum())
            total += int((a != b).sum())
        w.step()
        losses.append(w.mean_loss())
        torch.cuda.synchronize()
        keys, rows = _export(table)
        assert EMPTY not in keys and len(np.unique(keys)) == len(keys)
        # round t+1's pull ran already and inserted its new keys: still at their
        # initial rows, and no part of this round's model
        nxt = np.unique(batches[(t + 1) % STEPS][0])
        early = ~np.isin(keys, np.union1d(sw.keys, np.unique(bk)))
        assert np.isin(keys[early], nxt).all()
        assert np.array_equal(rows[early, :dim], init_rows(keys[early]))
        assert (rows[early, dim:] == 0).all()
        keys, rows = keys[~early], rows[~early]
        sw.step(bk, y, keys, rows[:, :dim], rows[:, dim:2 * dim],
                pulled=None if pulled is None else pulled[1])
        order = np.argsort(keys)
        older, newer = newer, (keys[order], rows[order, :dim])
        if t + 1 < STEPS:
            pulled = _pulled_rows(w._pulled[0], batches[t + 1][0], dim)
    eng.check()
    table.check()
    print(f"PULLED SS_PULL_STREAM={pull_stream}: {fresh} of {total} pulled coordinates that push "
          f"i-1 changed already held its value")
    _check(f"pull-ahead replay SS_PULL_STREAM={pull_stream}", sw, [losses])


def _body_fm_worker_refuses_feature_values(tmp_path):
    """The FM kernels take binary features: a source with ``idx:val`` entries
    is refused at construction, not trained as if every value were 1."""
    dev, monkeypatch = _child_env()
    from swiftsnails_amd.models.fm import FMWorker
    from swiftsnails_amd.utils.dataio import FileCtrSource

    path = os.path.join(tmp_path, "valued.libsvm")
    open(path, "w").write("1 3:0.5 7:2.0\n0 4:1.5 9:0.25\n")
    src = FileCtrSource(path, batch_size=2, num_fields=2, resident="hbm", device=dev)
    assert src.has_values
    table = _table("adagrad", 9, dev)
    eng, _ = _engine("fast", table, dev, monkeypatch, "fm_spread")
    with pytest.raises(ValueError, match="binary features"):
        FMWorker(eng, src)


# ------------------------------------------------------- a process per case
class _Env:
    """monkeypatch's two calls, on this process's own environment."""

    @staticmethod
    def setenv(k, v):
        os.environ[k] = v

    @staticmethod
    def delenv(k, raising=False):
        os.environ.pop(k, None)


def _child_env():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    return dev, _Env


def _fresh(fn, *args):
    """A case's body in a spawned process of its own (the module docstring
    says why)."""
    in_child(fn, *args, always=True)


# the tests: each runs its body (above) in a process of its own
def test_device_init_within_the_relative_term():
    _fresh(_body_device_init_within_the_relative_term)


@pytest.mark.parametrize("dim,optimizer", [(2, "adagrad"), (5, "adagrad"), (9, "adagrad"),
                                           (17, "adagrad"), (9, "sgd")])
def test_fm_fast_path_matches_fp64_oracle(files, dim, optimizer):
    _fresh(_body_fm_fast_path_matches_fp64_oracle, files, dim, optimizer)


@pytest.mark.parametrize("dim,optimizer", [(9, "sgd"), (17, "sgd"), (9, "adagrad"),
                                           (17, "adagrad")])
def test_fm_overflow_bucket_matches_fp64_oracle(files, dim, optimizer):
    _fresh(_body_fm_overflow_bucket_matches_fp64_oracle, files, dim, optimizer)


@pytest.mark.parametrize("name,dim,dedup", [("fm_spread", 9, "hash"), ("fm_spread", 17, "hash"),
                                            ("fm_narrow", 17, None)])
def test_fm_row_atomic_fallback_matches_fp64_oracle(files, name, dim, dedup):
    _fresh(_body_fm_row_atomic_fallback_matches_fp64_oracle, files, name, dim, dedup)


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_fm_xgmi_unique_world1_matches_fp64_oracle(files, optimizer):
    _fresh(_body_fm_xgmi_unique_world1_matches_fp64_oracle, files, optimizer)


def test_fm_bf16_rows(files):
    _fresh(_body_fm_bf16_rows, files)


@pytest.mark.parametrize("pull_stream", ["0", "1"])
def test_fm_pull_ahead_replay_matches_fp64_oracle(files, pull_stream):
    _fresh(_body_fm_pull_ahead_replay_matches_fp64_oracle, files, pull_stream)


def test_fm_worker_refuses_feature_values(tmp_path):
    _fresh(_body_fm_worker_refuses_feature_values, str(tmp_path))
