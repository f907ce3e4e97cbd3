"""The field-aware FM through the paths it trains on, against the fp64 oracle
of ``_ffm_oracle.py``.

Built like ``test_gpu_fm_paths_oracle.py``: every case runs in a spawned
process of its own (the open cross-test defect recorded there and in
``docs/TESTING.md``), trains eight synchronous rounds from an HBM-resident
``FileCtrSource`` over the helper's libsvm files, whose batches are checked bit
for bit against the arrays the oracle steps on (the EMPTY gaps keep every
occurrence at its column: ``field_by_rank`` would show here), and is held to
``_ffm_oracle.Stepwise`` after every round.  The rows are planted: the table's
``InitConfig`` is the helper's (scale per data set, AdaGrad state 0.01), new
keys take their rows from a scratch table with the same ``InitConfig``.

Asserted in every case: each step's summed loss within its bound, the exported
key set exactly, every coordinate of x and h within the derived bound (no
``1e-4 |x|`` term), untouched keys bit-identical, the diagonal blocks equal to
their initial bits after the last step, no ill-conditioned key-step on the
engine's own trajectory, and what ran (``eng.fast1``, ``eng.xg``, the dedup
mode).  SGD cases are also held to the free-running reference with its carried
bound.

Cases: the fast path on the three data sets with AdaGrad and SGD; the shipped
initialiser with ``CtrSynth`` (a state of 0; no ill-conditioned key-step,
asserted); ``SS_DEDUP=hash``; the xGMI
unique exchange at world 1 on ``ffm_mid`` and ``ffm_wide`` (157-float rows
through the arena); bf16 rows on ``ffm_mid`` and ``ffm_wide`` (every stored
word a bf16 neighbour of [oracle - bound, oracle + bound]); checkpoint, text
round trip and ``resize`` of the 314-float rows of ``ffm_wide``, then two more
steps of the reloaded table; the fast path from an AdaGrad state of 0 on the
three data sets (the count of ill-conditioned key-steps asserted against the
fp64 reference from the same rows); the xGMI unique exchange at world 2 on one
GPU against the union-batch oracle; pull-ahead as ``FFMWorker`` ships it, as a
replay from the rows actually pulled; hipGraph replay on ``CtrSynth`` with SGD
against the free-running reference and an eager twin.

Each case prints ``MARGIN ...``: the largest |engine - oracle| / bound;
``docs/TESTING.md`` has the figures measured on an MI355X.
"""
import os

import numpy as np
import pytest
import torch

import torch.distributed as dist
import torch.multiprocessing as mp

import _ffm_oracle as O
import _opt_oracle as _opt
from _lr_oracle import EMPTY
from _mp import collect, file_init, in_child, init_gloo

pytestmark = pytest.mark.gpu

KNOBS = ("SS_CLAIM", "SS_SLOT32", "SS_TABLE_REGIONS", "SS_ENGINE_GENERAL", "SS_DEDUP",
         "SS_XGMI_SELF", "SS_SERVER_STREAM", "SS_STALENESS", "SS_ENGINE_DEPTH",
         "SS_TABLE_G", "SS_PULL_STREAM")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ffm_oracle")
    return {n: O.dataset(n).write(d / f"{n}.libsvm") for n in O.F}


def _all_keys(name):
    k = np.unique(O.dataset(name).keys)
    return k[k != EMPTY]


def _capacity(n_keys):
    """The smallest power of two that keeps the load below 0.7."""
    return 1 << int(np.ceil(np.log2(n_keys / 0.7)))


def _table(name, optimizer, dev, row_dtype="fp32", capacity=None, state0=False):
    from swiftsnails_amd.ops.optim import InitConfig, Optimizer
    from swiftsnails_amd.ops.table import HbmTable

    dim = 1 + O.F[name] * O.K[name]
    init = InitConfig("normal", scale=O.INIT_SCALE[name],
                      state_init=O.STATE_INIT if optimizer == "adagrad" and not state0 else 0.0)
    return HbmTable(dim, capacity or _capacity(len(_all_keys(name))),
                    optimizer=Optimizer(optimizer, lr=O.LR[optimizer], eps=O.EPS), init=init,
                    device=dev, row_dtype=row_dtype)


def _init_rows(name, dev, row_dtype="fp32"):
    """keys -> the device's initial parameters, read once from a scratch table."""
    keys = _all_keys(name)
    t = _table(name, "sgd", dev, row_dtype)
    rows, _ = t.pull(torch.from_numpy(keys.view(np.int64)).to(dev))
    torch.cuda.synchronize()
    t.check()
    rows = rows.cpu().numpy()

    def f(k):
        pos = np.searchsorted(keys, k)
        assert np.array_equal(keys[pos], k)
        return rows[pos]
    return f


def _source(path, name, dev):
    """The HBM-resident file source, its batches checked bit for bit against
    the arrays the oracle steps on."""
    from swiftsnails_amd.utils.dataio import FileCtrSource

    ds, nf, B = O.dataset(name), O.F[name], O.BATCH[name]
    src = FileCtrSource(path, batch_size=B, num_fields=nf, resident="hbm", device=dev)
    assert src.rows == B * O.STEPS and not src.has_values
    k = torch.empty(B * nf, dtype=torch.int64, device=dev)
    y = torch.empty(B, dtype=torch.float32, device=dev)
    for t in range(O.STEPS):
        src.generate(t, 0, 1, k, y)
        ek, _, ey = ds.batch(t, B)
        assert np.array_equal(k.cpu().numpy().view(np.uint64), ek.reshape(-1)), t
        assert np.array_equal(y.cpu().numpy(), ey), t
    return src


def _engine(path, table, dev, max_keys, dedup=None, pull_ahead="0"):
    from swiftsnails_amd.parallel.engine import PSEngine
    from swiftsnails_amd.parallel.xgmi import XgmiTransport

    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.pop("SS_PULL_AHEAD", None)
    if pull_ahead is not None:
        os.environ["SS_PULL_AHEAD"] = pull_ahead
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    if dedup:
        os.environ["SS_DEDUP"] = dedup
    tr = None if path == "fast" else XgmiTransport(0, 1, dev, None, timeout_s=30)
    return PSEngine(table, tr, max_keys=max_keys, dim=table.dim, device=dev), tr


def _export(table):
    ks, rs = [], []
    for k, r in table.export():
        ks.append(k.numpy())
        rs.append(r.numpy())
    keys, rows = np.concatenate(ks).view(np.uint64), np.concatenate(rs)
    order = np.argsort(keys)
    return keys[order], rows[order]


def _dev():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    return dev


def _diagonal(keys, rows, first_field, K):
    """Each key's diagonal block, by the one field it ever occurred in (keys
    seen in one field only)."""
    f = first_field(keys)
    ok = f >= 0
    cols = 1 + f[ok, None] * K + np.arange(K)[None, :]
    return ok, rows[np.nonzero(ok)[0][:, None], cols]


def _single_field(name):
    """keys -> the field of a key that occurs in one column only, else -1."""
    ds = O.dataset(name)
    r, c = np.nonzero(ds.keys != EMPTY)
    k = ds.keys[r, c]
    order = np.lexsort((c, k))
    k, c = k[order], c[order]
    u, start = np.unique(k, return_index=True)
    lo, hi = c[start], c[np.append(start[1:], len(k)) - 1]
    field = np.where(lo == hi, lo, -1)

    def f(keys):
        return field[np.searchsorted(u, keys)]
    return f


def _check(label, sw, check_ill=True):
    print(f"MARGIN {label}: max |engine - oracle| / bound  x {sw.rx:.3f}  h {sw.rh:.3f}  "
          f"loss {sw.rl:.3f}  (ill-conditioned key-steps {sw.ill}, max |z| {sw.zmax:.1f})")
    if check_ill:
        assert sw.ill == 0
    assert sw.rx <= 1 and sw.rh <= 1 and sw.rl <= 1, (label, sw.rx, sw.rh, sw.rl, sw.out)


def _run(label, files, name, optimizer, path="fast", dedup=None, state0=False):
    from swiftsnails_amd.models.ffm import FFMWorker

    dev = _dev()
    nf, K, B = O.F[name], O.K[name], O.BATCH[name]
    D, ada = 1 + nf * K, optimizer == "adagrad"
    table = _table(name, optimizer, dev, state0=state0)
    eng, tr = _engine(path, table, dev, B * nf, dedup)
    w = FFMWorker(eng, _source(files[name], name, dev), K)
    assert not eng.pull_ahead and table.width == (2 * D if ada else D)
    if path == "fast":
        assert eng.fast1 and eng.xg is None
    else:
        assert not eng.fast1 and eng.xg is not None
    assert all(dd.mode == (dedup or "bucket") for dd in eng.dedupers)
    init_rows = _init_rows(name, dev)
    h0 = 0.0 if state0 else O.state_init(optimizer)
    sw = O.Stepwise(nf, K, optimizer, O.LR[optimizer], init_rows, state_init=h0)
    for bk, y in O.batches(name):
        loss = float(w.step().sum().item())
        torch.cuda.synchronize()
        keys, rows = _export(table)
        assert EMPTY not in keys and len(np.unique(keys)) == len(keys)  # one slot per key
        sw.step(bk, y, keys, rows[:, :D], rows[:, D:2 * D] if ada else None, loss=loss)
    eng.check()
    table.check()
    if tr is not None:
        tr.close()
    if state0:
        # the ill-conditioned key-steps are the ones the fp64 reference has from
        # the same initial rows, no more: the monotone bound holds those alone
        ref = O.FFMOracle(nf, K, optimizer, O.LR[optimizer], init_rows=init_rows)
        for bk, y in O.batches(name):
            ref.step(bk, y)
        print(f"ILL {label}: engine's trajectory {sw.ill}, fp64 reference {ref.ill}, "
              f"host-mirror reference {O.ILL_FROM_STATE_0[name]}")
        assert sw.ill == ref.ill <= O.ILL_FROM_STATE_0[name] + 2
    _check(label, sw, check_ill=not state0)
    ok, diag = _diagonal(keys, rows[:, :D], _single_field(name), K)
    assert ok.sum() > len(keys) // 2
    want = _diagonal(keys, init_rows(keys), _single_field(name), K)[1]
    assert np.array_equal(diag.view(np.uint32), want.view(np.uint32))  # never written
    if not ada:
        fk, fx, ftol = O.free_running(name, init_rows)
        assert np.array_equal(fk, keys)
        d = np.abs(rows[:, :D].astype(np.float64) - fx)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(d == 0, 0.0, d / ftol).max())
        print(f"MARGIN {label} free-running: max |engine - oracle| / bound  x {r:.3f}")
        assert r <= 1


def _body_fast(files, name, optimizer):
    _run(f"fast {name} {optimizer}", files, name, optimizer)


def _body_hash(files):
    _run("SS_DEDUP=hash ffm_mid adagrad", files, "ffm_mid", "adagrad", dedup="hash")


def _body_xgmi1(files, name, optimizer):
    _run(f"xgmi unique world 1 {name} {optimizer}", files, name, optimizer, path="unique")


def _body_shipped_initialiser():
    """``ffm_table_args``' rows (normal 0.01, state 0) with ``CtrSynth``."""
    from swiftsnails_amd.models.ffm import FFMWorker, ffm_table_args
    from swiftsnails_amd.models.sparse_lr import CtrSynth
    from swiftsnails_amd.ops.optim import Optimizer
    from swiftsnails_amd.ops.table import HbmTable

    dev = _dev()
    B, nf, K = 512, 13, 4
    D = 1 + nf * K
    data = CtrSynth(batch_size=B, num_fields=nf, num_features=3000, tail_frac=0.0)
    opt, init = ffm_table_args(K, Optimizer("adagrad", lr=0.05, eps=O.EPS))
    assert (init.kind, init.scale, init.state_init) == ("normal", 0.01, 0.0)
    table = HbmTable(D, 1 << 14, optimizer=opt, init=init, device=dev)
    eng, _ = _engine("fast", table, dev, B * nf)
    w = FFMWorker(eng, data, K)
    assert eng.fast1 and not eng.pull_ahead
    scratch = HbmTable(D, 1 << 14, optimizer=Optimizer("sgd"), init=init, device=dev)

    def init_rows(k):
        return scratch.pull(torch.from_numpy(k.view(np.int64)).to(dev))[0].cpu().numpy()

    sw = O.Stepwise(nf, K, "adagrad", 0.05, init_rows)
    tk, ty = torch.empty(B * nf, dtype=torch.int64, device=dev), torch.empty(B, device=dev)
    for step in range(O.STEPS):
        data.generate(step, 0, 1, tk, ty)
        bk, y = tk.cpu().numpy().view(np.uint64).reshape(B, nf), ty.cpu().numpy()
        loss = float(w.step().sum().item())
        torch.cuda.synchronize()
        keys, rows = _export(table)
        sw.step(bk, y, keys, rows[:, :D], rows[:, D:], loss=loss)
    table.check()
    _check("shipped initialiser CtrSynth adagrad", sw)  # no ill-conditioned key-step from state 0


def _body_bf16(files, name):
    """bf16 rows (fp32 math, stochastically rounded stores): every stored word
    is a bf16 neighbour of [oracle - bound, oracle + bound], step by step from
    the table's own rows; none outside."""
    from swiftsnails_amd.models.ffm import FFMWorker

    dev = _dev()
    nf, K, B = O.F[name], O.K[name], O.BATCH[name]
    D = 1 + nf * K
    table = _table(name, "adagrad", dev, row_dtype="bf16")
    eng, _ = _engine("fast", table, dev, B * nf)
    w = FFMWorker(eng, _source(files[name], name, dev), K)
    assert eng.fast1
    fp32_init = _init_rows(name, dev)

    def init_rows(k):
        """A compact row holds its initial values rounded to bf16, to nearest even."""
        u = fp32_init(k).view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32)

    sw = O.Stepwise(nf, K, "adagrad", O.LR["adagrad"], init_rows,
                    state_init=O.state_init("adagrad", "bf16"))
    outside = total = 0
    for bk, y in O.batches(name):
        loss = float(w.step().sum().item())
        torch.cuda.synchronize()
        keys, rows = _export(table)
        sw.step(bk, y, keys, rows[:, :D], rows[:, D:], loss=loss, compare=False)
        pos, xr, hr, tx, th = sw.last
        for got, ref, tol in ((rows[pos, :D], xr, tx), (rows[pos, D:], hr, th)):
            lo, hi = _opt.bf16_interval(ref - tol, ref + tol)
            outside += int(((got < lo) | (got > hi)).sum())
            total += got.size
    table.check()
    print(f"MARGIN bf16 rows {name}: {outside} of {total} stored words outside the bf16 "
          f"neighbours of [oracle - bound, oracle + bound]; loss {sw.rl:.3f}")
    assert sw.ill == 0 and outside == 0 and sw.rl <= 1


def _body_checkpoint(files, tmp):
    """314-float rows: binary and with-state text round trips and ``resize``,
    bit for bit; the reloaded table then trains on within the oracle's bound."""
    from swiftsnails_amd.models.ffm import FFMWorker
    from swiftsnails_amd.utils import checkpoint as ck

    dev = _dev()
    name, optimizer = "ffm_wide", "adagrad"
    nf, K, B = O.F[name], O.K[name], O.BATCH[name]
    D = 1 + nf * K
    table = _table(name, optimizer, dev)
    assert table.width == 314
    eng, _ = _engine("fast", table, dev, B * nf)
    w = FFMWorker(eng, _source(files[name], name, dev), K)
    init_rows = _init_rows(name, dev)
    sw = O.Stepwise(nf, K, optimizer, O.LR[optimizer], init_rows,
                    state_init=O.state_init(optimizer))
    batches = O.batches(name)
    for bk, y in batches[:4]:
        loss = float(w.step().sum().item())
        torch.cuda.synchronize()
        keys, rows = _export(table)
        sw.step(bk, y, keys, rows[:, :D], rows[:, D:], loss=loss)
    table.check()

    def same(t):
        k2, r2 = _export(t)
        return np.array_equal(k2, keys) and np.array_equal(r2.view(np.uint32), rows.view(np.uint32))

    pb, pt = os.path.join(tmp, "ffm.bin"), os.path.join(tmp, "ffm.txt")
    assert ck.save_binary(table, pb) == len(keys)
    ck.save_text(table, pt, precision=9, with_state=True)
    tb, tt = _table(name, optimizer, dev), _table(name, optimizer, dev)
    assert ck.load_binary(tb, pb) == len(keys) and same(tb)
    assert ck.load_text(tt, pt) == len(keys) and same(tt)
    tb.resize(2 * tb.capacity)
    tb.check()
    assert tb.capacity == 2 * table.capacity and same(tb)
    eng2, _ = _engine("fast", tb, dev, B * nf)
    w2 = FFMWorker(eng2, _source(files[name], name, dev), K)
    w2.step_idx = 4
    for bk, y in batches[4:6]:
        loss = float(w2.step().sum().item())
        torch.cuda.synchronize()
        k2, r2 = _export(tb)
        sw.step(bk, y, k2, r2[:, :D], r2[:, D:], loss=loss)
    tb.check()
    _check("checkpoint, resize and resume ffm_wide adagrad", sw)


def _body_state0(files, name):
    _run(f"fast {name} adagrad from state 0", files, name, "adagrad", state0=True)


# ------------------------------------------------------------------ world 2
def _rank(rank, world, path, name, optimizer, init, q):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ["SS_PULL_AHEAD"] = "0"
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    init_gloo(init, rank, world)
    try:
        from swiftsnails_amd.models.ffm import FFMWorker
        from swiftsnails_amd.parallel.engine import PSEngine
        from swiftsnails_amd.parallel.transport import TorchDistTransport
        from swiftsnails_amd.parallel.xgmi import XgmiTransport
        from swiftsnails_amd.utils.dataio import FileCtrSource

        dev = _dev()
        ds, nf, K, B = O.dataset(name), O.F[name], O.K[name], O.BATCH[name] // world
        tr = XgmiTransport(rank, world, dev, dist.distributed_c10d._get_default_store(),
                           aux=TorchDistTransport(), timeout_s=30)
        table = _table(name, optimizer, dev)
        eng = PSEngine(table, tr, max_keys=B * nf, dim=table.dim, device=dev)
        src = FileCtrSource(path, batch_size=B, num_fields=nf, rank=rank, world=world,
                            resident="hbm", device=dev)
        lo, hi = ds.shard(rank, world)
        assert src.rows == hi - lo
        k = torch.empty(B * nf, dtype=torch.int64, device=dev)
        y = torch.empty(B, dtype=torch.float32, device=dev)
        for t in range(O.STEPS):  # this rank's batches, bit for bit
            src.generate(t, rank, world, k, y)
            ek, _, ey = ds.batch(t, B, rank, world)
            assert np.array_equal(k.cpu().numpy().view(np.uint64), ek.reshape(-1)), t
            assert np.array_equal(y.cpu().numpy(), ey), t
        w = FFMWorker(eng, src, K, rank=rank, world=world)
        flags = {"fast1": bool(eng.fast1), "xg": eng.xg is not None,
                 "records": bool(eng.records), "ahead": bool(eng.pull_ahead)}
        irows = None
        if rank == 0:  # the device's initial rows, for the parent's oracle
            keys = _all_keys(name)
            irows = (keys, _init_rows(name, dev)(keys))
        losses, snaps = [], []
        for _ in range(O.STEPS):
            losses.append(float(w.step().sum().item()))
            torch.cuda.synchronize()
            dist.barrier()  # both ranks' pushes of this round are applied
            snaps.append(_export(table))
            dist.barrier()
        eng.check()
        table.check()
        q.put((rank, losses, snaps, flags, irows))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_ffm_world2_matches_fp64_oracle(files, optimizer):
    """Two ranks on one GPU, each reading its half of the file: a synchronous
    round is one update per key on the sum of both ranks' gradients, the
    world-1 update of the union batch."""
    world, name = 2, "ffm_mid"
    nf, K = O.F[name], O.K[name]
    D, ada = 1 + nf * K, optimizer == "adagrad"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    init = file_init()
    procs = [ctx.Process(target=_rank, args=(r, world, files[name], name, optimizer, init, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = collect(q, procs, world, 180)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort(key=lambda x: x[0])
    for _, _, _, f, _ in res:
        assert not f["fast1"] and f["xg"] and not f["records"] and not f["ahead"]
    ikeys, irows = res[0][4]

    def init_rows(k):
        pos = np.searchsorted(ikeys, k)
        assert np.array_equal(ikeys[pos], k)
        return irows[pos]

    sw = O.Stepwise(nf, K, optimizer, O.LR[optimizer], init_rows,
                    state_init=O.state_init(optimizer))
    worst = 0.0
    for t, (bk, y) in enumerate(O.batches(name, world)):
        keys = np.concatenate([r[2][t][0] for r in res])
        rows = np.concatenate([r[2][t][1] for r in res])
        assert all(len(r[2][t][0]) > 0 for r in res)  # both shards hold keys
        assert EMPTY not in keys and len(np.unique(keys)) == len(keys)
        g = sw.step(bk, y, keys, rows[:, :D], rows[:, D:2 * D] if ada else None)
        # each rank's summed loss: its half of the union batch, with the whole batch's bound
        half = g.loss.astype(np.float64).reshape(world, -1).sum(1)
        for r in range(world):
            worst = max(worst, abs(res[r][1][t] - half[r]) / g.tol_loss)
    sw.rl = worst
    _check(f"world 2 xgmi unique {name} {optimizer}", sw)
    if not ada:
        fk, fx, ftol = O.free_running(name, init_rows, world)
        order = np.argsort(keys)
        assert np.array_equal(fk, keys[order])
        d = np.abs(rows[order, :D].astype(np.float64) - fx)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.where(d == 0, 0.0, d / ftol).max())
        print(f"MARGIN world 2 xgmi unique {name} sgd free-running: x {r:.3f}")
        assert r <= 1


# --------------------------------------------------------------- pull-ahead
def _pulled_rows(rnd, bk, D):
    """The rows a pulled round holds, by key: (sorted distinct keys of the
    batch, their rows), every occurrence of a key resolving to one row."""
    flat = bk.reshape(-1)
    uid = rnd.inv[:flat.size].cpu().numpy().view(np.uint32).astype(np.int64)
    live = uid != 0xFFFFFFFF
    assert np.array_equal(live, flat != EMPTY)
    u, first, inv = np.unique(flat[live], return_index=True, return_inverse=True)
    ids = uid[live]
    assert np.array_equal(ids, ids[first][inv]) and len(np.unique(ids[first])) == len(u)
    return u, rnd.uvals[torch.from_numpy(ids[first]).to(rnd.uvals.device)].cpu().numpy()[:, :D]


def _body_pull_ahead(files, name):
    """Pull-ahead as ``FFMWorker`` ships it.  The pull of round i is enqueued
    before push i-1 and waits only for push i-2, so each pulled coordinate is
    bit-identical to the table after push i-2 or after push i-1; the oracle
    replays every round from the rows actually pulled, and the table after
    every push must match the replay."""
    from swiftsnails_amd.models.ffm import FFMWorker

    dev = _dev()
    nf, K, B = O.F[name], O.K[name], O.BATCH[name]
    D = 1 + nf * K
    table = _table(name, "adagrad", dev)
    eng, _ = _engine("fast", table, dev, B * nf, pull_ahead=None)
    w = FFMWorker(eng, _source(files[name], name, dev), K)
    assert eng.fast1 and eng.pull_ahead and eng.staleness == 1
    init_rows = _init_rows(name, dev)
    h0 = np.float32(O.state_init("adagrad"))
    sw = O.Stepwise(nf, K, "adagrad", O.LR["adagrad"], init_rows, state_init=float(h0))
    batches = O.batches(name)
    older = (np.empty(0, np.uint64), np.empty((0, D), np.float32))  # the table after push i-2
    newer = older                                                   # ... after push i-1
    pulled, fresh, total = None, 0, 0

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
        loss = float(w.step().sum().item())
        torch.cuda.synchronize()
        keys, rows = _export(table)
        assert EMPTY not in keys and len(np.unique(keys)) == len(keys)
        # round t+1's pull ran already and inserted its new keys: still at their
        # initial rows, and no part of this round's model
        nxt = np.unique(batches[(t + 1) % O.STEPS][0])
        early = ~np.isin(keys, np.union1d(sw.keys, np.unique(bk)))
        assert np.isin(keys[early], nxt).all()
        assert np.array_equal(rows[early, :D], init_rows(keys[early]))
        assert (rows[early, D:] == h0).all()
        keys, rows = keys[~early], rows[~early]
        sw.step(bk, y, keys, rows[:, :D], rows[:, D:], loss=loss,
                pulled=None if pulled is None else pulled[1])
        older, newer = newer, (keys, rows[:, :D])
        if t + 1 < O.STEPS:
            pulled = _pulled_rows(w._pulled[0], batches[t + 1][0], D)
    eng.check()
    table.check()
    print(f"PULLED {name}: {fresh} of {total} pulled coordinates that push i-1 changed already "
          f"held its value")
    _check(f"pull-ahead replay {name} adagrad", sw)


# ------------------------------------------------------------ hipGraph replay
def _body_graph():
    """``CtrSynth`` with SGD: one graph period of replayed steps, the final table
    held to the free-running fp64 reference with its carried bound and to an
    eager twin within the sum of both bounds.  If ``enable_graph()`` declines,
    that is asserted and printed."""
    from swiftsnails_amd.models.ffm import FFMWorker, ffm_table_args
    from swiftsnails_amd.models.sparse_lr import CtrSynth
    from swiftsnails_amd.ops.optim import Optimizer
    from swiftsnails_amd.ops.table import HbmTable

    dev = _dev()
    B, nf, K, lr = 512, 13, 4, 1e-3
    D = 1 + nf * K
    opt, init = ffm_table_args(K, Optimizer("sgd", lr=lr))

    def worker():
        data = CtrSynth(batch_size=B, num_fields=nf, num_features=3000, tail_frac=0.0)
        table = HbmTable(D, 1 << 14, optimizer=opt, init=init, device=dev)
        eng, _ = _engine("fast", table, dev, B * nf)
        return FFMWorker(eng, data, K), table, data

    wg, tg, data = worker()
    on = wg.enable_graph()
    print(f"GRAPH enable_graph() -> {on} (capturable source {data.graph_capturable}, "
          f"fast1 {wg.engine.fast1})")
    if not on:  # declined: recorded above; the eager path is every other case's
        assert wg._graphs is None
        return
    assert wg._graphs is not None and data.graph_capturable and wg.engine.fast1
    for _ in range(wg._gper):
        wg.step()
    torch.cuda.synchronize()
    n = wg.step_idx
    kg, xg = _export(tg)
    tg.check()
    wg.close()
    we, te, _ = worker()
    for _ in range(n):
        we.step()
    torch.cuda.synchronize()
    ke, xe = _export(te)
    te.check()
    scratch = HbmTable(D, 1 << 14, optimizer=Optimizer("sgd"), init=init, device=dev)

    def init_rows(k):
        return scratch.pull(torch.from_numpy(k.view(np.int64)).to(dev))[0].cpu().numpy()

    tk, ty = torch.empty(B * nf, dtype=torch.int64, device=dev), torch.empty(B, device=dev)
    source = []
    for t in range(n):
        data.generate(t, 0, 1, tk, ty)
        source.append((tk.cpu().numpy().view(np.uint64).reshape(B, nf).copy(),
                       ty.cpu().numpy().copy()))
    fk, fx, ftol = O.free_running(None, init_rows, source=source, nf=nf, k=K, lr=lr)
    assert np.array_equal(kg, fk) and np.array_equal(ke, fk)

    def ratio(d, tol):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.where(d == 0, 0.0, np.abs(d) / tol).max())

    rg, re = ratio(xg.astype(np.float64) - fx, ftol), ratio(xe.astype(np.float64) - fx, ftol)
    rt = ratio(xg.astype(np.float64) - xe, 2 * ftol)
    print(f"MARGIN hipGraph replay, {n} steps ({wg._gper} replayed): graph / reference {rg:.3f}  "
          f"eager / reference {re:.3f}  graph / eager {rt:.3f}")
    assert rg <= 1 and re <= 1 and rt <= 1


# the tests: each runs its body (above) in a process of its own
@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
@pytest.mark.parametrize("name", list(O.F))
def test_ffm_fast_path_matches_fp64_oracle(files, name, optimizer):
    in_child(_body_fast, files, name, optimizer, always=True)


def test_ffm_shipped_initialiser_matches_fp64_oracle():
    in_child(_body_shipped_initialiser, always=True)


def test_ffm_hash_dedup_matches_fp64_oracle(files):
    in_child(_body_hash, files, always=True)


@pytest.mark.parametrize("name,optimizer", [("ffm_mid", "adagrad"), ("ffm_mid", "sgd"),
                                            ("ffm_wide", "adagrad")])
def test_ffm_xgmi_unique_world1_matches_fp64_oracle(files, name, optimizer):
    in_child(_body_xgmi1, files, name, optimizer, always=True)


@pytest.mark.parametrize("name", ["ffm_mid", "ffm_wide"])
def test_ffm_bf16_rows(files, name):
    in_child(_body_bf16, files, name, always=True)


def test_ffm_checkpoint_resize_resume(files, tmp_path):
    in_child(_body_checkpoint, files, str(tmp_path), always=True)


@pytest.mark.parametrize("name", list(O.F))
def test_ffm_adagrad_from_state_0_matches_fp64_oracle(files, name):
    in_child(_body_state0, files, name, always=True)


@pytest.mark.parametrize("name", ["ffm_mid", "ffm_wide"])
def test_ffm_pull_ahead_replay_matches_fp64_oracle(files, name):
    in_child(_body_pull_ahead, files, name, always=True)


def test_ffm_hipgraph_replay_matches_fp64_oracle():
    in_child(_body_graph, always=True)
