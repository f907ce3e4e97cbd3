"""Sparse LR through every exchange against the fp64 oracle of ``_lr_oracle.py``.

``test_gpu_oracle.py`` holds one corner to an independent reference: binary
features, AdaGrad, the one-GPU fast path and the unique exchange.  Here the
same question — do the engine's rounds compute sparse LR? — is put to

* the one-GPU fast path, the xGMI **unique** exchange, and the **record**
  exchange with the rank's own records off the mailbox (``SS_REC_OCC=own``:
  cached own rows, the server merge reading ``g[spj[p] / F] * x[spj[p]]``) and
  through it (``arena``);
* **feature values** (``valued64``: ``idx:val`` entries reach ``k_bd_reduce``,
  ``k_rec_grad`` and the server merge's own segment; a quarter of the keys
  need 12-byte route records) and binary features (``binary32``);
* **AdaGrad and SGD**, a **tensor-code** rule (installed before and after
  the engine exists), **bf16** rows, and the server's gradient staging;
* **world 2** (two ranks on one GPU): rank 1's own segment sits at the
  non-zero offset ``rank * cap``.

The data are libsvm files the test writes (``FileCtrSource``, HBM-resident):
the loader's batches are checked bit for bit against the arrays the oracle
steps on.  Every case asserts the oracle's precondition (no ill-conditioned
key-step), each step's mean loss (rtol 1e-4), the exported key set (exactly
the oracle's: no EMPTY key, one slot per key) and every key's ``w`` and ``h``
within the oracle's own first-order tolerance (``tol_w`` / ``tol_h``,
calibrated on the CPU in ``test_lr_oracle_cpu.py``: no key excused, no
tolerance tuned to the kernels).

The record rounds with SGD, bf16 rows, a tensor-code rule or
``SS_SRV_STAGE=1`` used to raise ``push_xgmi: own_grad needs the fused scalar
merge, no staging`` — after the round's gradient put was enqueued: the engine
now takes the own-record shortcut only for rounds whose merge can read it
(``PSEngine.own_merge``).  Those cases must run, not raise.

Measured on an MI355X, the largest |engine - oracle| / tol per path (w, h;
each case prints its own as ``MARGIN ...``; reported, not tuned):

    fast path            0.062  0.166      records, own      0.055  0.164
    xGMI unique          0.043  0.166      records, arena    0.047  0.167
    tensor-code rule     0.009  -          world 2 (all 4)   0.009  0.030

The binary32 / AdaGrad cases set every maximum of h (0.164-0.167, all paths
alike, and 0.166 for the fp32 NumPy evaluation on the CPU): it is the fp32
noise floor of the model, not of a kernel.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _lr_oracle as O
from _mp import collect, file_init, init_gloo

pytestmark = pytest.mark.gpu

CAP = 1 << 22
KNOBS = ("SS_CLAIM", "SS_SLOT32", "SS_TABLE_REGIONS", "SS_ENGINE_GENERAL", "SS_DEDUP",
         "SS_REC_OCC", "SS_REC_GROUP", "SS_SRV_STAGE", "SS_XGMI_SELF", "SS_SERVER_STREAM",
         "SS_STALENESS", "SS_ENGINE_DEPTH", "SS_TABLE_G")
PATHS = ("fast", "unique", "records_own", "records_arena")


@pytest.fixture(scope="module")
def dev():
    from swiftsnails_amd._native import hip

    hip()  # loud failure if the extension is missing on a GPU box
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lr_oracle")
    return {n: O.dataset(n).write(d / f"{n}.libsvm") for n in ("binary32", "valued64")}


def _table(optimizer, dev, row_dtype="fp32"):
    from swiftsnails_amd.models.sparse_lr import lr_init, make_lr_table
    from swiftsnails_amd.ops.optim import Optimizer
    from swiftsnails_amd.ops.table import HbmTable

    opt = Optimizer(optimizer, lr=O.LR[optimizer], eps=O.EPS)
    init = lr_init("uniform", O.INIT_SCALE)
    if row_dtype != "fp32":
        return HbmTable(1, CAP, optimizer=opt, init=init, device=dev, row_dtype=row_dtype)
    return make_lr_table(2_000_003, 1, opt, device=dev, capacity=CAP, init=init)


def _source(path, name, batch, dev, rank=0, world=1):
    """The HBM-resident file source, its batches checked against the arrays
    the oracle steps on."""
    from swiftsnails_amd.utils.dataio import FileCtrSource

    ds = O.dataset(name)
    src = FileCtrSource(path, batch_size=batch, num_fields=O.F, rank=rank, world=world,
                        resident="hbm", device=dev)
    lo, hi = ds.shard(rank, world)
    assert src.rows == hi - lo and src.has_values == ds.has_values
    k = torch.empty(batch * O.F, dtype=torch.int64, device=dev)
    x = torch.empty(batch * O.F, dtype=torch.float32, device=dev)
    y = torch.empty(batch, dtype=torch.float32, device=dev)
    for t in range(O.STEPS):
        src.generate(t, rank, world, k, y, xval=x if src.has_values else None)
        ek, ex, ey = ds.batch(t, batch, rank, world)
        assert np.array_equal(k.cpu().numpy().view(np.uint64), ek.reshape(-1)), t
        assert np.array_equal(y.cpu().numpy(), ey), t
        if src.has_values:
            assert np.array_equal(x.cpu().numpy(), ex.reshape(-1)), t
    return src


def _engine(path, table, dev, monkeypatch):
    """The engine of one of PATHS at world 1 (knobs set before it is built)."""
    from swiftsnails_amd.parallel.engine import PSEngine
    from swiftsnails_amd.parallel.xgmi import XgmiTransport

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SS_PULL_AHEAD", "0")
    monkeypatch.setenv("SS_XGMI_TIMEOUT", "30")
    if path.startswith("records"):
        monkeypatch.setenv("SS_REC_OCC", path.split("_")[1])
    tr = None if path == "fast" else XgmiTransport(0, 1, dev, None, timeout_s=30)
    eng = PSEngine(table, tr, max_keys=O.B * O.F, dim=1, device=dev,
                   exchange="records" if path.startswith("records") else "unique")
    return eng, tr


def _train(w):
    losses = []
    for _ in range(O.STEPS):
        w.step()
        losses.append(w.mean_loss())
    torch.cuda.synchronize()
    return losses


def _export(table):
    ks, rs = [], []
    for k, r in table.export():
        ks.append(k.numpy())
        rs.append(r.numpy())
    return np.concatenate(ks).view(np.uint64), np.concatenate(rs)


def _check(label, ref, losses, keys, rows, world=1, with_h=True):
    """The assertions of every case; prints the margin before asserting it."""
    assert ref.ill == 0  # the oracle's precondition, from the oracle alone
    for r, l in enumerate(losses):
        np.testing.assert_allclose(l, ref.mean_losses(world)[:, r], rtol=1e-4)
    assert O.EMPTY not in keys and len(np.unique(keys)) == len(keys)  # one slot per key
    assert np.array_equal(np.sort(keys), ref.keys), (len(keys), len(ref.keys))
    rw, rh, out = O.ratios(ref, keys, rows[:, 0], rows[:, 1] if with_h else None)
    print(f"MARGIN {label}: max |engine - oracle| / tol  w {rw:.3f}  h {rh:.3f}")
    assert rw <= 1 and rh <= 1, (label, rw, rh, out)


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
@pytest.mark.parametrize("name", ["binary32", "valued64"])
@pytest.mark.parametrize("path", PATHS)
def test_lr_path_matches_fp64_oracle(dev, files, monkeypatch, path, name, optimizer):
    from swiftsnails_amd.models.sparse_lr import SparseLRWorker

    ada = optimizer == "adagrad"
    table = _table(optimizer, dev)
    assert table.rbits == (12 if ada else 0)
    eng, tr = _engine(path, table, dev, monkeypatch)
    w = SparseLRWorker(eng, _source(files[name], name, O.B, dev))
    assert (w.xval is not None) == (name == "valued64") and w.bucketed
    # the path under test is what runs
    if path == "fast":
        assert eng.fast1 and eng.claim == ada
    elif path == "unique":
        assert not eng.fast1 and eng.xg is not None and not eng.records
    elif path == "records_own":
        # the AdaGrad fp32 default keeps the own-record shortcut; SGD leaves it
        assert eng.records and eng.own_merge() == ada and (w.gring is not None or not ada)
    else:
        assert eng.records and w.gring is None and not eng.own_merge()
    losses = _train(w)
    eng.check()
    table.check()
    keys, rows = _export(table)
    if tr is not None:
        tr.close()
    _check(f"{path} {name} {optimizer}", O.reference(name, optimizer), [losses], keys, rows,
           with_h=ada)


C = O.LR["sgd"]


def _sgd_rule(rows, g):
    rows = rows.clone()
    rows[:, 0] -= C * g[:, 0]
    return rows


@pytest.mark.parametrize("when", ["before", "after"])
def test_records_own_tensor_code_rule(dev, files, monkeypatch, when):
    """A tensor-code update rule on the record exchange, installed before the
    engine is built and after it (the engine then holds the own-record buffers
    of the AdaGrad table it was built for): plain SGD with lr = c, h untouched."""
    from swiftsnails_amd.models.sparse_lr import SparseLRWorker

    table = _table("adagrad", dev)
    if when == "before":
        table.set_push_method(_sgd_rule)
    eng, tr = _engine("records_own", table, dev, monkeypatch)
    w = SparseLRWorker(eng, _source(files["valued64"], "valued64", O.B, dev))
    if when == "after":
        assert eng.own_merge() and w.gring is not None
        table.set_push_method(_sgd_rule)
    assert eng.records and not eng.own_merge()
    losses = _train(w)
    eng.check()
    table.check()
    keys, rows = _export(table)
    tr.close()
    assert (rows[:, 1] == 0).all()
    _check(f"records_own push_fn {when}", O.reference("valued64", "sgd"), [losses], keys, rows,
           with_h=False)


def test_records_own_bf16_rows(dev, files, monkeypatch):
    """Compact bf16 rows (stochastically rounded updates) on the record
    exchange: the oracle's key set exactly, rows within the bound
    ``test_compact_bf16_rows`` uses."""
    from swiftsnails_amd.models.sparse_lr import SparseLRWorker

    table = _table("adagrad", dev, row_dtype="bf16")
    eng, tr = _engine("records_own", table, dev, monkeypatch)
    w = SparseLRWorker(eng, _source(files["valued64"], "valued64", O.B, dev))
    assert eng.records and not eng.own_merge()
    losses = _train(w)
    eng.check()
    table.check()
    keys, rows = _export(table)
    tr.close()
    ref = O.reference("valued64", "adagrad")
    assert ref.ill == 0
    order = np.argsort(keys)
    assert np.array_equal(keys[order], ref.keys)
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    np.testing.assert_allclose(rows[order, 0], ref.w, rtol=0.03, atol=0.02)
    np.testing.assert_allclose(rows[order, 1], ref.h, rtol=0.03, atol=0.02)


# ------------------------------------------------------------------ world 2
def _rank(rank, world, path, name, optimizer, exchange, stage, init, q):
    os.environ["SS_PULL_AHEAD"] = "0"
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    os.environ["SS_SRV_STAGE"] = "1" if stage else "0"
    for k in KNOBS:
        if k != "SS_SRV_STAGE":
            os.environ.pop(k, None)
    init_gloo(init, rank, world)
    try:
        from swiftsnails_amd.models.sparse_lr import SparseLRWorker
        from swiftsnails_amd.parallel.engine import PSEngine
        from swiftsnails_amd.parallel.transport import TorchDistTransport
        from swiftsnails_amd.parallel.xgmi import XgmiTransport

        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        tr = XgmiTransport(rank, world, dev, dist.distributed_c10d._get_default_store(),
                           aux=TorchDistTransport(), timeout_s=30)
        table = _table(optimizer, dev)
        eng = PSEngine(table, tr, max_keys=O.B // world * O.F, dim=1, device=dev,
                       exchange=exchange)
        src = _source(path, name, O.B // world, dev, rank, world)
        w = SparseLRWorker(eng, src, rank=rank, world=world)
        flags = {"records": bool(eng.records), "own": bool(eng.own_merge()),
                 "gring": w.gring is not None, "stage": eng.gstage is not None,
                 "xval": w.xval is not None}
        losses = _train(w)
        eng.check()
        table.check()
        keys, rows = _export(table)
        q.put((rank, losses, keys, rows, flags))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("exchange,optimizer,stage", [
    ("records", "adagrad", False),   # rank 1's own segment at a non-zero offset
    ("unique", "adagrad", False),
    ("records", "sgd", False),
    ("records", "adagrad", True),    # SS_SRV_STAGE=1
])
def test_lr_world2_matches_fp64_oracle(files, exchange, optimizer, stage):
    """Two ranks on one GPU, each reading its half of the file: a synchronous
    round is one update per key on the sum of both ranks' gradients, the
    world-1 update of the union batch."""
    world, name = 2, "valued64"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    init = file_init()
    procs = [ctx.Process(target=_rank, args=(r, world, files[name], name, optimizer, exchange,
                                             stage, init, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(q, procs, world, 120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort(key=lambda x: x[0])
    ada = optimizer == "adagrad"
    for _, _, _, _, f in res:
        assert f["xval"] and f["records"] == (exchange == "records") and f["stage"] == stage
        # the AdaGrad fp32 default keeps the own-record path; staging and SGD leave it
        assert f["own"] == (exchange == "records" and ada and not stage)
        assert f["gring"] or not f["own"]
    keys = np.concatenate([x[2] for x in res])
    rows = np.concatenate([x[3] for x in res])
    assert all(len(x[2]) > 0 for x in res)  # both shards hold keys
    _check(f"world2 {exchange} {optimizer}{' staged' if stage else ''}",
           O.reference(name, optimizer, world), [x[1] for x in res], keys, rows, world=world,
           with_h=ada)
